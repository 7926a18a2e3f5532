// Output stage of CORRECT and CLEAN: the batch that lies in a handle (one or two planes of source bytes, input offsets `off`, one
// record per read) becomes the batch the next stage reads -- every read cut as its program cuts it (the corrector's trims,
// host/correct_error_reads.cpp:155,172; the cleaner's rule, dbgk_clean_rule.h), emptied reads of length 0 at their place, each
// plane back to back from a 16-byte boundary under one set of offsets.  Host side: dbgk_host_emit.h.
//
//   k_emit_out_len   one thread per read: its output length, the source byte its result starts at, and the numbers of the
//                    program's .stat file reduced per wave and per workgroup into 64-bit device counters.  What a record makes
//                    of its read is the template parameter: CorrRule, CleanRule<lowqual>, CleanRule<adapter>.
//   (scan)           lengths -> n + 1 compact offsets, 64 bit (dbgk_sort.hip, rocPRIM)
//   k_emit_gather    tiled by OUTPUT: a workgroup owns kEmitTile bytes of each plane, a lane one 16-byte vector of them.  Nothing
//                    goes through LDS.  The tile's reads [r0, r1) come from two 64-way searches in the compact offsets; a lane
//                    then finds the read that holds its first byte by bisection in coff[r0 .. r1) -- which passes over emptied
//                    reads without seeing them, so a run of 3 * TILE empty reads costs about 14 probes per lane.  An output
//                    dword that lies inside one read is composed in registers from the two aligned source dwords that hold its
//                    bytes (one when source and destination agree mod 4): a 64-bit shift, for the quality plane with the same
//                    addresses, and the N -> shift substitution as a byte mask computed from the composed base dword.  A dword
//                    that straddles a read boundary (or the end of the batch) is put together byte by byte; the read behind the
//                    current one is loaded ahead, so the change of read costs no dependent load unless empty reads lie between
//                    (then: bisection again).  Each plane is written with one aligned 16-byte store per lane.  Three forms:
//                    bases alone (a cleaner's batch without qualities), two planes, two planes with the substitution.
//   k_emit_gather_lds  the same job for ONE plane through a 4 KiB LDS tile, taken by the corrector's batches (at its definition)
//
// Known costs of the register gather.  (1) A lane's bisection is log2(r1 - r0) dependent loads of coff, served by L1/L2 (all lanes of a
// tile probe the same few lines) but not staged in LDS.  (2) Neighbouring output dwords of a lane share a source dword; it is
// loaded for both (8 dword loads per plane and lane where 5 would do) and left to L1.  (3) With reads of 150 bytes nearly every
// wave holds a lane with a straddling dword, so the wave issues the byte path too, for the few lanes that need it: about one
// dword in 37 takes it, but most waves pay its instructions.  None of the three has been profiled apart.  Measured:
// profiles/clean_handoff_measure.json (two planes), profiles/emit_merge_measure.json (one plane, the corrector's batches).
//
// Memory the gather reads: source bytes are read only inside [off[0] & ~3, off[n]) rounded up to whole dwords -- the second
// source dword of a pair is loaded only when it holds a byte of the read.  The planes are 16-byte aligned (the handles' own
// buffers are; the _device calls check it), so an aligned dword never leaves that range.
#pragma once

#include "dbgk_clean_rule.h"

namespace dbgk {
namespace emitk {

constexpr int kWave = 64;
constexpr int kEmitBlock = 256;
constexpr int kEmitTile = kEmitBlock * 16;
static_assert(DBGK_CORR_COMPACT_TILE == kEmitTile && DBGK_CLEAN_COMPACT_TILE == kEmitTile, "one 16-byte store per lane and plane writes a tile");

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
	for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
	return v;
}

// The N sums of one thread -> the device counters: per wave by shuffles, per workgroup in LDS, then one atomic per counter that is
// not 0.  Every thread of the workgroup calls it once (it holds barriers).
template <int N>
__device__ __forceinline__ void fold_counters(const unsigned long long (&v)[N], unsigned long long *__restrict__ counters)
{
	__shared__ unsigned long long part[N];
	if (threadIdx.x < N) part[threadIdx.x] = 0;
	__syncthreads();
#pragma unroll
	for (int c = 0; c < N; ++c) {
		const unsigned long long s = wave_sum(v[c]);
		if (lane_id() == 0 && s) atomicAdd(&part[c], s);
	}
	__syncthreads();
	if (threadIdx.x < N && part[threadIdx.x]) atomicAdd(&counters[threadIdx.x], part[threadIdx.x]);
}

// ---- what a record makes of its read ------------------------------------------------------------------------------------------------
// A rule is the kernel's argument.  read(t, i, L, start) -> the output length of read i of L bytes, the first kept byte in `start`
// (inside the read also when nothing is kept), the read added to the thread's tally t; t.sums(v) -> the tally as kCounters 64-bit
// sums in the order of the rule's enum, which is the order the host copies them into its info struct.

struct CorrRule {
	enum Counter {
		EC_RESULT_READS = 0, EC_RESULT_BASES, EC_TRIMMED_READS, EC_TRIMMED_BASES, EC_DELETED_READS, EC_ONE_BASE, EC_TREE,
		EC_NODE_LIMIT_HITS, EC_BY_CLASSIFY, EC_BY_CORRECT, EC_BY_OVERFLOW, EC_COUNT
	};
	static constexpr int kCounters = EC_COUNT;
	const dbgk_corr_rec *rec;

	// Output length of a read of L bytes.  The kernels of dbgk_correct.h mark a read deleted whenever L - left - right < -r
	// (r >= 0), so on their records left + right <= L holds for every read that is kept and the command line's unsigned
	// `L - left_trim - right_trim` never wraps; records from elsewhere (dbgk_corr_compact_from) that trim more than the read
	// holds give length 0, so that no byte outside the read is ever copied.
	static __device__ __forceinline__ uint32_t out_len(uint32_t L, const dbgk_corr_rec &q)
	{
		const uint64_t cut = (uint64_t)q.left_trim + q.right_trim;
		return (q.deleted || cut >= L) ? 0u : (uint32_t)(L - cut);
	}

	// sums of lengths and edits in 64 bits, counts of reads (at most 2^32 / the grid's threads) in 32
	struct Tally {
		unsigned long long bases = 0, cut = 0, one = 0, tree = 0, hits = 0;
		uint32_t kept = 0, trimmed = 0, deleted = 0, p0 = 0, p1 = 0, p2 = 0;
		__device__ __forceinline__ void sums(unsigned long long (&v)[EC_COUNT]) const
		{
			v[EC_RESULT_READS] = kept, v[EC_RESULT_BASES] = bases, v[EC_TRIMMED_READS] = trimmed, v[EC_TRIMMED_BASES] = cut;
			v[EC_DELETED_READS] = deleted, v[EC_ONE_BASE] = one, v[EC_TREE] = tree, v[EC_NODE_LIMIT_HITS] = hits;
			v[EC_BY_CLASSIFY] = p0, v[EC_BY_CORRECT] = p1, v[EC_BY_OVERFLOW] = p2;
		}
	};

	__device__ __forceinline__ uint32_t read(Tally &t, uint64_t i, uint32_t L, uint32_t &start) const
	{
		const dbgk_corr_rec q = rec[i];
		const uint32_t m = out_len(L, q);
		start = m ? q.left_trim : 0u; // (m > 0: left_trim + m <= L)
		if (q.deleted) {
			t.deleted++;
		} else {
			t.kept++;
			t.bases += m;
			t.one += q.one_base;
			t.tree += q.tree;
			if (q.left_trim > 0 || q.right_trim > 0) {
				t.trimmed++;
				t.cut += (unsigned long long)q.left_trim + q.right_trim;
			}
		}
		t.hits += q.node_limit_hits;
		t.p0 += q.path == 0;
		t.p1 += q.path == 1;
		t.p2 += q.path == 2;
		return m;
	}
};

// KIND: DBGK_CLEAN_KIND_*, the record type `rec` holds; the rule itself is dbgk_clean_rule.h
template <int KIND>
struct CleanRule {
	enum Counter { EC_RAW_BASES = 0, EC_TRIMMED_READS, EC_TRIMMED_BASES, EC_SHORT_READS, EC_SHORT_BASES, EC_CLEAN_READS, EC_CLEAN_BASES, EC_COUNT };
	static constexpr int kCounters = EC_COUNT;
	const void *rec;
	uint32_t min_len;

	struct Tally : cleank::CleanTally {
		__device__ __forceinline__ void sums(unsigned long long (&v)[EC_COUNT]) const
		{
			v[EC_RAW_BASES] = raw_bases, v[EC_TRIMMED_READS] = trimmed_reads, v[EC_TRIMMED_BASES] = trimmed_bases;
			v[EC_SHORT_READS] = short_reads, v[EC_SHORT_BASES] = short_bases, v[EC_CLEAN_READS] = clean_reads, v[EC_CLEAN_BASES] = clean_bases;
		}
	};

	// L < 2^30, checked by the host
	__device__ __forceinline__ uint32_t read(Tally &t, uint64_t i, uint32_t L, uint32_t &start) const
	{
		cleank::CleanCut cut;
		if (KIND == DBGK_CLEAN_KIND_LOWQUAL) {
			const cleank::LowqualBlock b = static_cast<const cleank::LowqualBlock *>(rec)[i];
			cut = cleank::clean_cut_lowqual(L, b.start, b.length, b.trimmed);
		} else {
			const cleank::AdapterHit h = static_cast<const cleank::AdapterHit *>(rec)[i];
			cut = cleank::clean_cut_adapter(L, h.adapter, h.read_start);
		}
		start = cut.start;
		return t.add(KIND, L, cut, min_len);
	}
};

// len[i] and src[i] (the byte of the source planes the result of read i starts at) for i < n; len[n] = 0: the scan runs over n + 1
// entries, its last output is the total
template <class Rule>
__global__ __launch_bounds__(kEmitBlock) void k_emit_out_len(const uint64_t *__restrict__ off, Rule rule, uint32_t n, uint32_t *__restrict__ len,
                                                             uint64_t *__restrict__ src, unsigned long long *__restrict__ counters)
{
	typename Rule::Tally t;
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i <= n; i += stride) {
		if (i == n) {
			len[i] = 0;
			break;
		}
		const uint64_t o = off[i];
		uint32_t start;
		len[i] = rule.read(t, i, (uint32_t)(off[i + 1] - o), start);
		src[i] = o + start;
	}
	unsigned long long v[Rule::kCounters];
	t.sums(v);
	fold_counters(v, counters);
}

// ---- the gather ---------------------------------------------------------------------------------------------------------------------

// First index in [0, count) at which a[idx + shift] > key (strict) or >= key (!strict), `count` if there is none; a is
// non-decreasing.  One wave, 64 probes a step: the range shrinks 64-fold per dependent load instead of 2-fold.
template <bool STRICT>
__device__ __forceinline__ uint64_t wave_search(const uint64_t *__restrict__ a, uint64_t shift, uint64_t count, uint64_t key, int lane)
{
	uint64_t lo = 0, hi = count; // the answer lies in [lo, hi]; index hi holds the condition or is `count`
	while (lo < hi) {
		const uint64_t step = (hi - lo + kWave - 1) / kWave; // [lo, hi) in 64 shares; a lane probes the last index of its share
		uint64_t probe = lo + ((uint64_t)lane + 1) * step - 1;
		if (probe > hi - 1) probe = hi - 1;
		const uint64_t x = a[probe + shift];
		const uint64_t hit = ballot(STRICT ? x > key : x >= key);
		if (!hit) break; // nothing in [lo, hi) holds
		const uint64_t f = (uint64_t)__ffsll((unsigned long long)hit) - 1; // the shares in front of share f do not hold, its last index does
		const uint64_t last = lo + (f + 1) * step - 1;
		lo += f * step;
		hi = last < hi - 1 ? last : hi - 1;
	}
	return hi;
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

// coff: n + 1 compact offsets, total = coff[n] > 0; src[r]: where the result of read r starts in seq / qual (never read for a read
// of length 0).  dst_b (and dst_q with QUAL) hold (total + 15) / 16 16-byte vectors, the pad of the last one is written as 0.
// SUBST: the quality of a base 'N' becomes the byte of shift_word (the shift in all four bytes).
template <bool QUAL, bool SUBST>
__global__ __launch_bounds__(kEmitBlock) void k_emit_gather(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual,
                                                            const uint64_t *__restrict__ src, const uint64_t *__restrict__ coff, uint32_t n,
                                                            uint64_t total, uint32_t shift_word, uint4 *__restrict__ dst_b,
                                                            uint4 *__restrict__ dst_q)
{
	static_assert(QUAL || !SUBST, "the substitution is made on the quality plane");
	__shared__ uint64_t range[2];
	const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid / kWave;
	const uint64_t n_tiles = (total + kEmitTile - 1) / kEmitTile;
	for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const uint64_t lo = t * kEmitTile, hi = lo + kEmitTile < total ? lo + kEmitTile : total;
		// reads [r0, r1) intersect [lo, hi): r0 = the first read that ends behind lo, r1 = the first that starts at or behind hi
		if (wave == 0) {
			const uint64_t r = wave_search<true>(coff, 1, n, lo, lane);
			if (lane == 0) range[0] = r;
		} else if (wave == 1) {
			const uint64_t r = wave_search<false>(coff, 0, (uint64_t)n + 1, hi, lane);
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

// The gather of ONE plane through an LDS tile: the corrector's batches take it, because on them it measures 2 % faster than
// k_emit_gather<false, false> (profiles/emit_merge_measure.json).  Same arguments, same result.  The reads of a tile are listed 256
// at a time: a pass is three barriers and one LDS atomic per read that holds bytes, so a run of 3 * TILE emptied reads inside a tile
// is 48 cheap passes -- parallel over the reads, never a walk of one lane.  A source word is one aligned 4-byte load and up to four
// ds_write_b8; the tile is read out with one 16-byte load and store per lane.
__global__ __launch_bounds__(kEmitBlock) void k_emit_gather_lds(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ src,
                                                                const uint64_t *__restrict__ coff, uint32_t n, uint64_t total,
                                                                uint4 *__restrict__ dst)
{
	__shared__ __attribute__((aligned(16))) uint8_t tile[kEmitTile];
	__shared__ uint32_t list[kEmitBlock];
	__shared__ uint32_t n_list;
	__shared__ uint64_t range[2];
	const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid / kWave;
	const uint64_t n_tiles = (total + kEmitTile - 1) / kEmitTile;
	for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const uint64_t lo = t * kEmitTile, hi = lo + kEmitTile < total ? lo + kEmitTile : total;
		// reads [r0, r1) intersect [lo, hi): r0 = the first read that ends behind lo, r1 = the first that starts at or behind hi
		if (wave == 0) {
			const uint64_t r = wave_search<true>(coff, 1, n, lo, lane);
			if (lane == 0) range[0] = r;
		} else if (wave == 1) {
			const uint64_t r = wave_search<false>(coff, 0, (uint64_t)n + 1, hi, lane);
			if (lane == 0) range[1] = r;
		}
		reinterpret_cast<uint4 *>(tile)[tid] = uint4{0, 0, 0, 0};
		__syncthreads();
		const uint64_t r0 = range[0], r1 = range[1] < n ? range[1] : n;
		for (uint64_t base = r0; base < r1; base += kEmitBlock) {
			// one pass over 256 reads: those that hold bytes go on the list (a run of emptied reads leaves it empty)
			if (tid == 0) n_list = 0;
			__syncthreads();
			const uint64_t i = base + tid;
			if (i < r1 && coff[i + 1] > coff[i]) list[atomicAdd(&n_list, 1u)] = (uint32_t)i;
			__syncthreads();
			const uint32_t m = n_list;
			// a read's piece: a wave along the read; with fewer pieces than waves, the whole workgroup along each
			const bool all = m < (uint32_t)(kEmitBlock / kWave);
			const uint32_t j0 = all ? 0u : (uint32_t)wave, dj = all ? 1u : (uint32_t)(kEmitBlock / kWave);
			const uint32_t w0 = all ? (uint32_t)tid : (uint32_t)lane, dw = all ? (uint32_t)kEmitBlock : (uint32_t)kWave;
			for (uint32_t j = j0; j < m; j += dj) {
				const uint32_t r = list[j];
				const uint64_t b = coff[r], e = coff[r + 1];
				const uint64_t ob = b > lo ? b : lo, oe = e < hi ? e : hi;          // the piece, in output bytes
				const uint64_t from = src[r] + (ob - b);                              // ... and where it lies in `seq`
				const uint32_t nbytes = (uint32_t)(oe - ob), at = (uint32_t)(ob - lo);
				const uint64_t a0 = from & ~3ull;
				const uint32_t head = (uint32_t)(from - a0), words = (head + nbytes + 3u) >> 2;
				for (uint32_t w = w0; w < words; w += dw) {
					const uint32_t x = *reinterpret_cast<const uint32_t *>(seq + a0 + 4ull * w);
#pragma unroll
					for (uint32_t k = 0; k < 4; ++k) {
						const uint32_t p = 4u * w + k; // byte of the piece's first word row; the piece is [head, head + nbytes)
						if (p >= head && p < head + nbytes) tile[at + p - head] = (uint8_t)(x >> (8u * k));
					}
				}
			}
			__syncthreads();
		}
		const uint64_t at = lo + 16ull * tid;
		if (at < total) dst[at >> 4] = reinterpret_cast<const uint4 *>(tile)[tid];
		__syncthreads(); // the tile and the range are rewritten by the next round
	}
}

} // namespace emitk
} // namespace dbgk
