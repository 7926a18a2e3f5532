// CORRECT, output stage: the corrected batch that lies in the handle (untrimmed bytes `out`, input offsets `off`, records
// `rec`) becomes the batch the next stage reads -- every read trimmed as the command line trims it
// (host/correct_error_reads.cpp:155,172), deleted reads of length 0 at their place, back to back from a 16-byte boundary.
//
//   k_corr_out_len   one thread per read: its output length, and the numbers of <file>.correct.stat / dbgk_corr_stats
//                    reduced per workgroup into 64-bit device counters
//   (scan)           lengths -> n + 1 compact offsets, 64 bit (dbgk_sort.hip, rocPRIM)
//   k_corr_gather    tiled by OUTPUT: a workgroup owns DBGK_CORR_COMPACT_TILE bytes of the compact buffer, finds the reads
//                    that intersect them with two searches in the compact offsets, collects their pieces in LDS and writes
//                    the tile with one aligned 16-byte store per lane
//
// Known cost of this first version of the gather.  The reads of a tile are listed 256 at a time: a pass is three barriers and one
// LDS atomic per read that holds bytes, so a run of 3 * TILE deleted reads inside a tile is 48 cheap passes -- parallel over the
// reads, never a walk of one lane, but not a single pass either.  A source word is one aligned 4-byte load and up to four
// ds_write_b8, i.e. per tile 64 wave-instructions of LDS byte stores against 4 for the 16-byte read-out.  Measured
// (profiles/handoff_measure.json) the kernel runs well below the copy rate; neither cost has been profiled apart.
#pragma once

namespace corr {

constexpr int kEmitBlock = 256;
static_assert(DBGK_CORR_COMPACT_TILE == kEmitBlock * 16, "one 16-byte store per lane writes a tile");

enum EmitCounter {
	EC_RESULT_READS = 0, EC_RESULT_BASES, EC_TRIMMED_READS, EC_TRIMMED_BASES, EC_DELETED_READS, EC_ONE_BASE, EC_TREE,
	EC_NODE_LIMIT_HITS, EC_BY_CLASSIFY, EC_BY_CORRECT, EC_BY_OVERFLOW, EC_COUNT
};

// Output length of a read of L bytes.  The kernels of dbgk_correct.h mark a read deleted whenever L - left - right < -r
// (r >= 0), so on their records left + right <= L holds for every read that is kept and the command line's unsigned
// `L - left_trim - right_trim` never wraps; records from elsewhere (dbgk_corr_compact_from) that trim more than the read
// holds give length 0, so that no byte outside the read is ever copied.
__device__ __forceinline__ uint32_t out_len(uint32_t L, const dbgk_corr_rec &q)
{
	const uint64_t cut = (uint64_t)q.left_trim + q.right_trim;
	return (q.deleted || cut >= L) ? 0u : (uint32_t)(L - cut);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
	for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
	return v;
}

// len[i] for i < n, len[n] = 0 (the scan runs over n + 1 entries: its last output is the total)
__global__ __launch_bounds__(kEmitBlock) void k_corr_out_len(const uint64_t *__restrict__ off, const dbgk_corr_rec *__restrict__ rec,
                                                             uint32_t n, uint32_t *__restrict__ len, unsigned long long *__restrict__ counters)
{
	__shared__ unsigned long long part[EC_COUNT];
	if (threadIdx.x < EC_COUNT) part[threadIdx.x] = 0;
	__syncthreads();
	// per thread: sums of lengths and edits in 64 bits, counts of reads (at most 2^32 / the grid's threads) in 32
	unsigned long long bases = 0, cut = 0, one = 0, tree = 0, hits = 0;
	uint32_t kept = 0, trimmed = 0, deleted = 0, p0 = 0, p1 = 0, p2 = 0;
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i <= n; i += stride) {
		if (i == n) {
			len[i] = 0;
			break;
		}
		const dbgk_corr_rec q = rec[i];
		const uint32_t L = (uint32_t)(off[i + 1] - off[i]), m = out_len(L, q);
		len[i] = m;
		if (q.deleted) {
			deleted++;
		} else {
			kept++;
			bases += m;
			one += q.one_base;
			tree += q.tree;
			if (q.left_trim > 0 || q.right_trim > 0) {
				trimmed++;
				cut += (unsigned long long)q.left_trim + q.right_trim;
			}
		}
		hits += q.node_limit_hits;
		p0 += q.path == 0;
		p1 += q.path == 1;
		p2 += q.path == 2;
	}
	auto fold = [&](int c, unsigned long long v) {
		const unsigned long long s = wave_sum(v);
		if (lane_id() == 0 && s) atomicAdd(&part[c], s);
	};
	fold(EC_RESULT_READS, kept);
	fold(EC_RESULT_BASES, bases);
	fold(EC_TRIMMED_READS, trimmed);
	fold(EC_TRIMMED_BASES, cut);
	fold(EC_DELETED_READS, deleted);
	fold(EC_ONE_BASE, one);
	fold(EC_TREE, tree);
	fold(EC_NODE_LIMIT_HITS, hits);
	fold(EC_BY_CLASSIFY, p0);
	fold(EC_BY_CORRECT, p1);
	fold(EC_BY_OVERFLOW, p2);
	__syncthreads();
	if (threadIdx.x < EC_COUNT && part[threadIdx.x]) atomicAdd(&counters[threadIdx.x], part[threadIdx.x]);
}

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

// coff: n + 1 compact offsets; total = coff[n] > 0; dst holds (total + 15) / 16 16-byte vectors, the pad of the last one is
// written as 0.  Source bytes are read as aligned 32-bit words: `out` is readable from its 4-byte-aligned start through the
// word that holds its last byte (the handle's buffers are, dbgk_host_correct.h).
__global__ __launch_bounds__(kEmitBlock) void k_corr_gather(const uint8_t *__restrict__ out, const uint64_t *__restrict__ off,
                                                            const dbgk_corr_rec *__restrict__ rec, const uint64_t *__restrict__ coff,
                                                            uint32_t n, uint64_t total, uint4 *__restrict__ dst)
{
	__shared__ __attribute__((aligned(16))) uint8_t tile[DBGK_CORR_COMPACT_TILE];
	__shared__ uint32_t list[kEmitBlock];
	__shared__ uint32_t n_list;
	__shared__ uint64_t range[2];
	const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid / kWave;
	const uint64_t n_tiles = (total + DBGK_CORR_COMPACT_TILE - 1) / DBGK_CORR_COMPACT_TILE;
	for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const uint64_t lo = t * DBGK_CORR_COMPACT_TILE, hi = lo + DBGK_CORR_COMPACT_TILE < total ? lo + DBGK_CORR_COMPACT_TILE : total;
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
			// one pass over 256 reads: those that hold bytes go on the list (a run of deleted reads leaves it empty)
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
				const uint64_t src = off[r] + rec[r].left_trim + (ob - b);            // ... and where it lies in `out`
				const uint32_t nbytes = (uint32_t)(oe - ob), at = (uint32_t)(ob - lo);
				const uint64_t a0 = src & ~3ull;
				const uint32_t head = (uint32_t)(src - a0), words = (head + nbytes + 3u) >> 2;
				for (uint32_t w = w0; w < words; w += dw) {
					const uint32_t x = *reinterpret_cast<const uint32_t *>(out + a0 + 4ull * w);
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

} // namespace corr
