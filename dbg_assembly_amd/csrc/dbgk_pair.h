// PAIR stage: two compact batches of n reads each (mate 1 and mate 2 of pair i at index i, the layout dbgk_emit.h writes) become
// the two batches an assembly run keeps -- PAIR: mate 1 then mate 2 of every pair whose mates are both not empty, SINGLE: the one
// mate that is left of every other pair -- in index order, in that same layout.  This is merge_two_corr_files
// (correct_error/correct.cpp:851-922) as data movement.  Host side: dbgk_host_pair.h.
//
//   k_pair_classify  one thread per pair: its class as two flags (kept in PAIR, kept in SINGLE), and the counters -- pair reads,
//                    pair bases, single reads, single bases, reads no 32-bit length can hold -- reduced per wave and workgroup
//                    as fold_counters does; the longest read by a wave maximum and one atomic per wave that saw a read.
//   (scan)           each flag plane -> the number of kept pairs in front of pair i (dbgk_sort.hip, rocPRIM): rank
//   k_pair_scatter   one thread per pair: length, source start (bit 63: the read lies in the planes of mate 2) and source id
//                    2 i + mate of its reads to rank 2 * rank_pair[i] (+ 1) of PAIR or rank_single[i] of SINGLE.
//   (scan)           lengths -> compact offsets of either output
//   k_pair_gather    k_emit_gather with TWO source planes per output plane: tiled by output bytes, one aligned 16-byte store per
//                    lane and plane, a dword inside one read composed in registers from the aligned source dwords that hold it,
//                    a dword that straddles reads byte by byte.  What changes with the read is one 64-bit address per plane
//                    (source plane + source start - output start) instead of one delta; the two searches, the bisection and the
//                    composition are dbgk_emit.h's.
//
// Memory the gather reads: source bytes only inside the whole dwords of [off[0] & ~3, off[n]) of each input plane, as the emit
// gather promises; the planes are 16-byte aligned (checked by the host), so an aligned dword never leaves that range.
//
// Known costs, none profiled apart: the three of the emit gather (dbgk_emit.h); the rank is two scans over 4-byte flags where
// one pass with a decoupled look-back would do; k_pair_scatter reads the input offsets a second time.
#pragma once

#include "dbgk_emit.h"

namespace dbgk {
namespace pairk {

using emitk::kEmitBlock;
using emitk::kEmitTile;
using emitk::kWave;

constexpr uint64_t kPlane2 = 1ull << 63; // in a source start: the read lies in the planes of mate 2
enum Counter { PC_PAIR_READS = 0, PC_PAIR_BASES, PC_SINGLE_READS, PC_SINGLE_BASES, PC_BAD, PC_SUMS, PC_MAX_LEN = PC_SUMS, PC_COUNT };

// flag_p[i] / flag_s[i] for i < n, 0 at i == n (the scans run over n + 1 entries, their last output is the count)
__global__ __launch_bounds__(kEmitBlock) void k_pair_classify(const uint64_t *__restrict__ off1, const uint64_t *__restrict__ off2, uint32_t n,
                                                              uint32_t *__restrict__ flag_p, uint32_t *__restrict__ flag_s,
                                                              unsigned long long *__restrict__ counters)
{
	// sums of lengths in 64 bits, counts of reads (at most 2^32 / the grid's threads) and the longest read (< 2^31) in 32
	unsigned long long pair_bases = 0, single_bases = 0;
	uint32_t pair_reads = 0, single_reads = 0, bad = 0, longest = 0;
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
#pragma unroll 1
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i <= n; i += stride) {
		if (i == n) {
			flag_p[i] = flag_s[i] = 0;
			break;
		}
		const uint64_t l1 = off1[i + 1] - off1[i], l2 = off2[i + 1] - off2[i];
		if ((l1 | l2) >> 31) { // decreasing offsets, or a read the 32-bit lengths cannot hold: the host refuses the batch
			bad++;
			flag_p[i] = flag_s[i] = 0;
			continue;
		}
		const bool both = l1 && l2, one = !both && (l1 | l2);
		flag_p[i] = both;
		flag_s[i] = one;
		if (both) {
			pair_reads += 2;
			pair_bases += l1 + l2;
		} else if (one) {
			single_reads += 1;
			single_bases += l1 | l2;
		}
		longest = max(longest, (uint32_t)max(l1, l2));
	}
	for (int d = kWave / 2; d > 0; d >>= 1) longest = max(longest, (uint32_t)__shfl_down(longest, d, kWave));
	if (emitk::lane_id() == 0 && longest) atomicMax(&counters[PC_MAX_LEN], (unsigned long long)longest);
	const unsigned long long v[PC_SUMS] = {pair_reads, pair_bases, single_reads, single_bases, bad};
	emitk::fold_counters(v, counters);
}

struct PairOut {
	uint32_t *len;  // reads + 1 lengths, the last one 0
	uint64_t *src;  // where each read starts in its source planes, | kPlane2
	uint32_t *id;   // 2 i + mate
};

// rank_p / rank_s: the exclusive scans of the flags over n + 1 entries
__global__ __launch_bounds__(kEmitBlock) void k_pair_scatter(const uint64_t *__restrict__ off1, const uint64_t *__restrict__ off2, uint32_t n,
                                                             const uint64_t *__restrict__ rank_p, const uint64_t *__restrict__ rank_s, PairOut P,
                                                             PairOut S)
{
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i <= n; i += stride) {
		if (i == n) {
			P.len[2 * rank_p[n]] = 0;
			S.len[rank_s[n]] = 0;
			break;
		}
		const uint64_t o1 = off1[i], o2 = off2[i];
		const uint64_t l1 = off1[i + 1] - o1, l2 = off2[i + 1] - o2;
		if ((l1 | l2) >> 31) continue;
		if (l1 && l2) {
			const uint64_t r = 2 * rank_p[i];
			P.len[r] = (uint32_t)l1;
			P.src[r] = o1;
			P.id[r] = (uint32_t)(2 * i);
			P.len[r + 1] = (uint32_t)l2;
			P.src[r + 1] = o2 | kPlane2;
			P.id[r + 1] = (uint32_t)(2 * i + 1);
		} else if (l1 | l2) {
			const uint64_t r = rank_s[i];
			S.len[r] = (uint32_t)(l1 | l2);
			S.src[r] = l1 ? o1 : (o2 | kPlane2);
			S.id[r] = (uint32_t)(2 * i + (l1 ? 0 : 1));
		}
	}
}

// the four bytes from byte address a on, all of them inside a batch whose plane is 16-byte aligned
__device__ __forceinline__ uint32_t load_unaligned_at(uint64_t a)
{
	const uint64_t a0 = a & ~3ull;
	const uint32_t sh = (uint32_t)(a - a0);
	const uint32_t w0 = *reinterpret_cast<const uint32_t *>(a0);
	const uint32_t w1 = sh ? *reinterpret_cast<const uint32_t *>(a0 + 4) : 0u; // (without a byte of it wanted it may lie behind the batch)
	return (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8u * sh));
}

// the planes of both mates; q1 / q2 are read with QUAL only
struct PairPlanes {
	const uint8_t *b1, *b2, *q1, *q2;
	// output byte p of a read that starts at output byte c and at source start s (| kPlane2) is the byte at address base + p
	__device__ __forceinline__ uint64_t base_b(uint64_t s, uint64_t c) const
	{
		return (uint64_t)((s & kPlane2) ? b2 : b1) + (s & ~kPlane2) - c;
	}
	__device__ __forceinline__ uint64_t base_q(uint64_t s, uint64_t c) const
	{
		return (uint64_t)((s & kPlane2) ? q2 : q1) + (s & ~kPlane2) - c;
	}
};

// coff: n + 1 compact offsets of the output, total = coff[n] > 0; src[r]: as k_pair_scatter wrote it (never read for a read of
// length 0: the outputs hold none, but nothing here depends on that).  dst_b (and dst_q with QUAL) hold (total + 15) / 16 16-byte
// vectors, the pad of the last one is written as 0.
template <bool QUAL>
__global__ __launch_bounds__(kEmitBlock) void k_pair_gather(PairPlanes in, const uint64_t *__restrict__ src, const uint64_t *__restrict__ coff,
                                                            uint32_t n, uint64_t total, uint4 *__restrict__ dst_b, uint4 *__restrict__ dst_q)
{
	__shared__ uint64_t range[2];
	const int tid = (int)threadIdx.x, lane = emitk::lane_id(), wave = tid / kWave;
	const uint64_t n_tiles = (total + kEmitTile - 1) / kEmitTile;
	for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const uint64_t lo = t * kEmitTile, hi = lo + kEmitTile < total ? lo + kEmitTile : total;
		// reads [r0, r1) intersect [lo, hi): r0 = the first read that ends behind lo, r1 = the first that starts at or behind hi
		if (wave == 0) {
			const uint64_t r = emitk::wave_search<true>(coff, 1, n, lo, lane);
			if (lane == 0) range[0] = r;
		} else if (wave == 1) {
			const uint64_t r = emitk::wave_search<false>(coff, 0, (uint64_t)n + 1, hi, lane);
			if (lane == 0) range[1] = r;
		}
		__syncthreads();
		const uint64_t r0 = range[0], r1 = range[1] < n ? range[1] : n;
		const uint64_t pos = lo + 16ull * tid;
		if (pos < hi) {
			uint64_t r = emitk::owner_of(coff, r0, r1, pos);
			uint64_t e = coff[r + 1]; // the read ends at output byte e
			uint64_t ab, aq = 0;      // output byte p is the byte at address ab + p (aq + p in the quality plane)
			{
				const uint64_t s = src[r], c = coff[r];
				ab = in.base_b(s, c);
				if (QUAL) aq = in.base_q(s, c);
			}
			// the read behind it, loaded beside the values above: where read r ends, read r + 1 takes over without a dependent load
			// unless it is empty
			uint64_t e2 = r + 2 <= n ? coff[r + 2] : e, s2 = r + 1 < n ? src[r + 1] : 0;
			uint32_t vb[4], vq[4];
#pragma unroll
			for (int d = 0; d < 4; ++d) {
				const uint64_t p = pos + 4u * d;
				uint32_t xb = 0, xq = 0;
				if (p + 4 <= e) { // the dword lies inside the read (its first byte does: every path below leaves p < e or p >= hi)
					xb = load_unaligned_at(ab + p);
					if (QUAL) xq = load_unaligned_at(aq + p);
				} else {
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						const uint64_t q = p + k;
						if (q >= hi) break; // behind the batch: the pad stays 0 (a tile ends on a dword unless the batch ends in it)
						if (q >= e) {      // the next read that holds bytes: read r + 1, or the one found behind a run of empty reads
							uint64_t s, c;
							if (q < e2) {
								r += 1;
								s = s2;
								c = e;
								e = e2;
							} else {
								r = emitk::owner_of(coff, r + 1, r1, q);
								e = coff[r + 1];
								s = src[r];
								c = coff[r];
							}
							ab = in.base_b(s, c);
							if (QUAL) aq = in.base_q(s, c);
							e2 = r + 2 <= n ? coff[r + 2] : e;
							s2 = r + 1 < n ? src[r + 1] : 0;
						}
						xb |= (uint32_t)*reinterpret_cast<const uint8_t *>(ab + q) << (8 * k);
						if (QUAL) xq |= (uint32_t)*reinterpret_cast<const uint8_t *>(aq + q) << (8 * k);
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

} // namespace pairk
} // namespace dbgk
