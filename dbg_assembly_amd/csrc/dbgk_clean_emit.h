// CLEAN, output stage: the batch that lies in the handle (bases `seq`, qualities `qual`, input offsets `off`, one record per read)
// becomes the batch the next stage reads -- every read cut as the two programs cut it (dbgk_clean_rule.h), emptied reads of
// length 0 at their place, both planes back to back from a 16-byte boundary under one set of offsets.
//
//   k_clean_out_len   one thread per read: its output length, the source byte its result starts at, and the numbers of the .stat
//                     file reduced per wave and per workgroup into 64-bit device counters.  The record type is the template
//                     parameter.
//   (scan)            lengths -> n + 1 compact offsets, 64 bit (dbgk_sort.hip, rocPRIM)
//   k_clean_gather    tiled by OUTPUT: a workgroup owns DBGK_CLEAN_COMPACT_TILE bytes of each plane, a lane one 16-byte vector
//                     of them.  Nothing goes through LDS.  The tile's reads [r0, r1) come from the two 64-way searches of the
//                     corrector's gather; a lane then finds the read that holds its first byte by bisection in coff[r0 .. r1) --
//                     which passes over emptied reads without seeing them, so there is no listing pass and a run of 3 * TILE
//                     empty reads costs about 14 probes per lane instead of 5.  An output dword that lies inside one read is
//                     composed in registers from the two aligned source dwords that hold its bytes (one when source and
//                     destination agree mod 4): a 64-bit shift, for the quality plane with the same addresses, and the N -> shift
//                     substitution as a byte mask computed from the composed base dword.  A dword that straddles a read boundary
//                     (or the end of the batch) is put together byte by byte; the read behind the current one is loaded ahead,
//                     so the change of read costs no dependent load unless empty reads lie between (then: bisection again).
//                     Each plane is written with one aligned 16-byte store per lane.
//
// Known costs of this shape.  (1) A lane's bisection is log2(r1 - r0) dependent loads of coff, served by L1/L2 (all lanes of a
// tile probe the same few lines) but not staged in LDS.  (2) Neighbouring output dwords of a lane share a source dword; it is
// loaded for both (8 dword loads per plane and lane where 5 would do) and left to L1.  (3) With reads of 150 bytes nearly every
// wave holds a lane with a straddling dword, so the wave issues the byte path too, for the few lanes that need it: about one
// dword in 37 takes it, but most waves pay its instructions.  None of the three has been profiled apart.  Measured
// (profiles/clean_handoff_measure.json): 1.43 TB/s of bytes read + written on two planes, a quarter of the copy rate and 1.3 times
// k_corr_gather on one plane of the same output size.
//
// Memory the gather reads: source bytes are read only inside [off[0] & ~3, off[n]) rounded up to whole dwords -- the second
// source dword of a pair is loaded only when it holds a byte of the read.  The planes are 16-byte aligned (the handle's own
// buffers are; the _device calls check it), so an aligned dword never leaves that range.
#pragma once

#include "dbgk_clean_rule.h"

namespace dbgk {
namespace cleank {

constexpr int kEmitBlock = 256;
static_assert(DBGK_CLEAN_COMPACT_TILE == kEmitBlock * 16, "one 16-byte store per lane and plane writes a tile");

enum EmitCounter { EC_RAW_BASES = 0, EC_TRIMMED_READS, EC_TRIMMED_BASES, EC_SHORT_READS, EC_SHORT_BASES, EC_CLEAN_READS, EC_CLEAN_BASES, EC_COUNT };

template <int KIND>
__device__ __forceinline__ CleanCut cut_of(const void *__restrict__ rec, uint64_t i, uint32_t L)
{
	if (KIND == DBGK_CLEAN_KIND_LOWQUAL) {
		const LowqualBlock b = static_cast<const LowqualBlock *>(rec)[i];
		return clean_cut_lowqual(L, b.start, b.length, b.trimmed);
	}
	const AdapterHit h = static_cast<const AdapterHit *>(rec)[i];
	return clean_cut_adapter(L, h.adapter, h.read_start);
}

// len[i] and src[i] (the byte of `seq` / `qual` the result of read i starts at) for i < n; len[n] = 0: the scan runs over n + 1
// entries, its last output is the total
template <int KIND>
__global__ __launch_bounds__(kEmitBlock) void k_clean_out_len(const uint64_t *__restrict__ off, const void *__restrict__ rec, uint32_t n,
                                                              uint32_t min_len, uint32_t *__restrict__ len, uint64_t *__restrict__ src,
                                                              unsigned long long *__restrict__ counters)
{
	__shared__ unsigned long long part[EC_COUNT];
	if (threadIdx.x < EC_COUNT) part[threadIdx.x] = 0;
	__syncthreads();
	CleanTally t;
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i <= n; i += stride) {
		if (i == n) {
			len[i] = 0;
			break;
		}
		const uint64_t o = off[i];
		const uint32_t L = (uint32_t)(off[i + 1] - o); // < 2^30, checked by the host
		const CleanCut cut = cut_of<KIND>(rec, i, L);
		len[i] = t.add(KIND, L, cut, min_len);
		src[i] = o + cut.start;
	}
	auto fold = [&](int c, unsigned long long v) {
		const unsigned long long s = corr::wave_sum(v);
		if (corr::lane_id() == 0 && s) atomicAdd(&part[c], s);
	};
	fold(EC_RAW_BASES, t.raw_bases);
	fold(EC_TRIMMED_READS, t.trimmed_reads);
	fold(EC_TRIMMED_BASES, t.trimmed_bases);
	fold(EC_SHORT_READS, t.short_reads);
	fold(EC_SHORT_BASES, t.short_bases);
	fold(EC_CLEAN_READS, t.clean_reads);
	fold(EC_CLEAN_BASES, t.clean_bases);
	__syncthreads();
	if (threadIdx.x < EC_COUNT && part[threadIdx.x]) atomicAdd(&counters[threadIdx.x], part[threadIdx.x]);
}

// the last index r in [a, r1) with coff[r] <= q; coff[a] <= q < coff[r1].  Among reads that start at one offset this is the last
// one, the only one of them that can hold bytes.
__device__ __forceinline__ uint64_t owner_of(const uint64_t *__restrict__ coff, uint64_t a, uint64_t r1, uint64_t q)
{
	uint64_t lo = a, hi = r1;
	while (hi - lo > 1) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		if (coff[mid] <= q) lo = mid;
		else hi = mid;
	}
	return lo;
}

// 0xFF in every byte of the result where the byte of x is 'N', 0 elsewhere (exact: no carry runs from one byte into the next)
__device__ __forceinline__ uint32_t n_bytes_mask(uint32_t x)
{
	const uint32_t y = x ^ 0x4E4E4E4Eu; // a zero byte where x holds 'N'
	const uint32_t nz = ((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y; // bit 7 of a byte set: that byte of y is not zero
	return ((~nz & 0x80808080u) >> 7) * 0xFFu;
}

// the four bytes from byte address s of p on (p 16-byte aligned), all of them inside the batch
__device__ __forceinline__ uint32_t load_unaligned(const uint8_t *__restrict__ p, uint64_t s)
{
	const uint64_t a0 = s & ~3ull;
	const uint32_t sh = (uint32_t)(s - a0);
	const uint32_t w0 = *reinterpret_cast<const uint32_t *>(p + a0);
	const uint32_t w1 = sh ? *reinterpret_cast<const uint32_t *>(p + a0 + 4) : 0u; // (without a byte of it wanted it may lie behind the batch)
	return (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8u * sh));
}

// coff: n + 1 compact offsets, total = coff[n] > 0; src[r]: where the result of read r starts in seq / qual.  dst_b (and dst_q with
// QUAL) hold (total + 15) / 16 16-byte vectors, the pad of the last one is written as 0.  SUBST: the quality of a base 'N' becomes
// the byte of shift_word (the shift in all four bytes).
template <bool QUAL, bool SUBST>
__global__ __launch_bounds__(kEmitBlock) void k_clean_gather(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual,
                                                             const uint64_t *__restrict__ src, const uint64_t *__restrict__ coff, uint32_t n,
                                                             uint64_t total, uint32_t shift_word, uint4 *__restrict__ dst_b,
                                                             uint4 *__restrict__ dst_q)
{
	static_assert(QUAL || !SUBST, "the substitution is made on the quality plane");
	__shared__ uint64_t range[2];
	const int tid = (int)threadIdx.x, lane = corr::lane_id(), wave = tid / corr::kWave;
	const uint64_t n_tiles = (total + DBGK_CLEAN_COMPACT_TILE - 1) / DBGK_CLEAN_COMPACT_TILE;
	for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const uint64_t lo = t * DBGK_CLEAN_COMPACT_TILE, hi = lo + DBGK_CLEAN_COMPACT_TILE < total ? lo + DBGK_CLEAN_COMPACT_TILE : total;
		// reads [r0, r1) intersect [lo, hi): r0 = the first read that ends behind lo, r1 = the first that starts at or behind hi
		if (wave == 0) {
			const uint64_t r = corr::wave_search<true>(coff, 1, n, lo, lane);
			if (lane == 0) range[0] = r;
		} else if (wave == 1) {
			const uint64_t r = corr::wave_search<false>(coff, 0, (uint64_t)n + 1, hi, lane);
			if (lane == 0) range[1] = r;
		}
		__syncthreads();
		const uint64_t r0 = range[0], r1 = range[1] < n ? range[1] : n;
		const uint64_t pos = lo + 16ull * tid;
		if (pos < hi) {
			uint64_t r = owner_of(coff, r0, r1, pos);
			uint64_t e = coff[r + 1], delta = src[r] - coff[r]; // the read ends at output byte e; output byte p is source byte p + delta
			// the read behind it, loaded beside the three values above: where read r ends, read r + 1 takes over without a dependent
			// load unless it is empty
			uint64_t e2 = r + 2 <= n ? coff[r + 2] : e, s2 = r + 1 < n ? src[r + 1] : 0;
			uint32_t vb[4], vq[4];
#pragma unroll
			for (int d = 0; d < 4; ++d) {
				const uint64_t p = pos + 4u * d;
				uint32_t xb = 0, xq = 0;
				if (p + 4 <= e) { // the dword lies inside the read (its first byte does: every path below leaves p < e or p >= hi)
					xb = load_unaligned(seq, p + delta);
					if (QUAL) xq = load_unaligned(qual, p + delta);
					if (SUBST) {
						const uint32_t m = n_bytes_mask(xb);
						xq = (xq & ~m) | (shift_word & m);
					}
				} else {
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						const uint64_t q = p + k;
						if (q >= hi) break; // behind the batch: the pad stays 0 (a tile ends on a dword unless the batch ends in it)
						if (q >= e) {      // the next read that holds bytes: read r + 1, or the one found behind a run of empty reads
							if (q < e2) {
								r += 1;
								delta = s2 - e;
								e = e2;
							} else {
								r = owner_of(coff, r + 1, r1, q);
								e = coff[r + 1];
								delta = src[r] - coff[r];
							}
							e2 = r + 2 <= n ? coff[r + 2] : e;
							s2 = r + 1 < n ? src[r + 1] : 0;
						}
						const uint32_t b = seq[q + delta];
						xb |= b << (8 * k);
						if (QUAL) xq |= (uint32_t)((SUBST && b == 'N') ? (shift_word & 0xFFu) : qual[q + delta]) << (8 * k);
					}
				}
				vb[d] = xb;
				vq[d] = xq;
			}
			dst_b[pos >> 4] = uint4{vb[0], vb[1], vb[2], vb[3]};
			if (QUAL) dst_q[pos >> 4] = uint4{vq[0], vq[1], vq[2], vq[3]};
		}
		__syncthreads(); // the range is rewritten by the next round
	}
}

} // namespace cleank
} // namespace dbgk
