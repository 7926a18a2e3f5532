// SUPER: kernels of link_supertig on the GPU (include/dbgk.h, SUPER section; host side in dbgk_host_super.h).
//
// The link table is FILL's (k_fill_orient, then the LINK sort / reduce / chain).  What link_supertig adds is its own gap statistics
// and the read slices that span every gap.  One stable radix sort by the unordered contig pair puts the records of a pair side by
// side in file order; k_super_gapstat reduces every pair to sum, minimum, maximum and count of its gaps (pass 0) and to the sum of
// the deviations from the truncated mean (pass 1), k_super_gappack writes one PairStat per pair.  The slices of the layout are
// cut out of the reads by k_super_slices, back to back in the order *.supertig.gap.data lists them.
#pragma once
#include <stdint.h>

namespace superk {

constexpr int kSuperThreads = 256;
constexpr int kWave = 64;
constexpr uint32_t kPieceBytes = 1024;         // a slice is copied in pieces of at most this many bytes, one wavefront each

struct Acc {                                   // the running statistics of the pair whose first sorted record is at this position
	unsigned long long sum;                    // of the gaps, two's complement
	unsigned long long dev;                    // of |mean - gap|
	uint32_t max_b;                            // largest gap ^ 0x80000000 (0 when no record has arrived)
	uint32_t min_b;                            // largest ~(gap ^ 0x80000000)
	uint32_t count, pad;
};
struct PairStat {                              // one contig pair (decide_gap_size, link_supertig.cpp:561-605) before the divisions
	uint64_t key;                              // contig_lo << 32 | contig_hi
	int64_t sum, dev;
	int32_t min, max;
	uint32_t total, pad;
	uint64_t first;                            // position of the pair's first record in the sorted array
};
struct Piece {                                 // at most kPieceBytes bytes of one slice
	uint64_t src;                              // first byte read: the piece's first byte, or its LAST byte when rev (read backwards)
	uint64_t dst;
	uint32_t len, rev;
};
struct Counters {
	unsigned long long pairs;                  // slots handed out by k_super_gappack
};

// the position of the first record of the run of equal keys that holds position at (keys[at - 1] == keys[at]): gallop back, bisect
__device__ __forceinline__ uint64_t super_run_begin(const uint64_t *__restrict__ keys, uint64_t at)
{
	const uint64_t key = keys[at];
	uint64_t hi = at, lo, step = 1;                // keys[hi] == key
	for (;;) {
		if (hi < step) {
			if (keys[0] == key) return 0;
			lo = 0;
			break;
		}
		if (keys[hi - step] != key) { lo = hi - step; break; }
		hi -= step;
		step *= 2;
	}
	while (hi - lo > 1) {                          // keys[lo] != key
		const uint64_t mid = lo + (hi - lo) / 2;
		if (keys[mid] == key) hi = mid; else lo = mid;
	}
	return hi;
}

// Segmented reduce over the records sorted by pair, a tile of 256 records per block round.  Every thread learns the position of its
// pair's first record (an inclusive max-scan of the head positions of the tile; a pair that began before the tile is traced back by
// one thread), the wavefront folds the values of equal pairs with shuffles, and the first lane of each pair in a wavefront adds
// its part to the pair's accumulator.  PASS 0: sum, min, max, count.  PASS 1: sum of |mean - gap| around mean = sum / count, the
// division truncating toward zero as the reference's int division does.
template <int PASS>
__global__ __launch_bounds__(kSuperThreads) void k_super_gapstat(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ vals, uint64_t n,
                                                                 Acc *__restrict__ acc)
{
	__shared__ uint64_t s_wave_head[kSuperThreads / kWave];
	__shared__ uint64_t s_before;
	const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
	const uint64_t none = ~0ull;
	for (uint64_t base = (uint64_t)blockIdx.x * kSuperThreads; base < n; base += (uint64_t)gridDim.x * kSuperThreads) {
		const uint64_t i = base + threadIdx.x;
		const bool live = i < n;
		uint64_t key = 0;
		int32_t gap = 0;
		bool head = false;
		if (live) {
			key = keys[i];
			gap = (int32_t)(uint32_t)vals[i];
			head = i == 0 || keys[i - 1] != key;
		}
		if (threadIdx.x == 0) s_before = head ? i : super_run_begin(keys, i);   // (base < n: thread 0 is live)
		// the last head at or before this thread, within the wavefront
		uint64_t hpos = head ? i : none;
		for (int off = 1; off < kWave; off *= 2) {
			const uint64_t o = __shfl_up(hpos, off);
			if (lane >= (uint32_t)off && hpos == none) hpos = o;
		}
		if (lane == kWave - 1) s_wave_head[wave] = hpos;
		__syncthreads();
		if (hpos == none) {
			for (int w = (int)wave - 1; w >= 0 && hpos == none; --w) hpos = s_wave_head[w];
			if (hpos == none) hpos = s_before;
		}
		// fold equal pairs: afterwards lane l holds the values of lanes l .. end of its pair in this wavefront
		long long sum = 0;
		uint32_t mx = 0, mn = 0, cnt = 0;
		if (live) {
			if (PASS == 0) {
				sum = gap;
				mx = (uint32_t)gap ^ 0x80000000u;
				mn = ~mx;
				cnt = 1;
			} else {
				const Acc a = acc[hpos];
				const long long mean = (long long)a.sum / (long long)a.count;
				const long long d = mean - (long long)gap;
				sum = d < 0 ? -d : d;
			}
		}
		const uint64_t seg = live ? hpos : none;
		for (int off = 1; off < kWave; off *= 2) {
			const uint64_t oseg = __shfl_down(seg, off);
			const long long osum = __shfl_down(sum, off);
			const uint32_t omx = __shfl_down(mx, off), omn = __shfl_down(mn, off), ocnt = __shfl_down(cnt, off);
			if (lane + (uint32_t)off < (uint32_t)kWave && oseg == seg) {
				sum += osum;
				if (PASS == 0) {
					mx = omx > mx ? omx : mx;
					mn = omn > mn ? omn : mn;
					cnt += ocnt;
				}
			}
		}
		const uint64_t pseg = __shfl_up(seg, 1);
		if (live && (lane == 0 || pseg != seg)) {
			Acc *a = acc + hpos;
			if (PASS == 0) {
				atomicAdd(&a->sum, (unsigned long long)sum);
				atomicMax(&a->max_b, mx);
				atomicMax(&a->min_b, mn);
				atomicAdd(&a->count, cnt);
			} else {
				atomicAdd(&a->dev, (unsigned long long)sum);
			}
		}
		__syncthreads();                               // s_before and s_wave_head are written again in the next round
	}
}

// one PairStat per pair, in no particular order
__global__ __launch_bounds__(kSuperThreads) void k_super_gappack(const uint64_t *__restrict__ keys, uint64_t n, const Acc *__restrict__ acc,
                                                                 PairStat *__restrict__ out, Counters *ctr)
{
	for (uint64_t i = (uint64_t)blockIdx.x * kSuperThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSuperThreads) {
		const uint64_t key = keys[i];
		if (i > 0 && keys[i - 1] == key) continue;
		const Acc a = acc[i];
		PairStat s;
		s.key = key;
		s.sum = (int64_t)a.sum;
		s.dev = (int64_t)a.dev;
		s.max = (int32_t)(a.max_b ^ 0x80000000u);
		s.min = (int32_t)(~a.min_b ^ 0x80000000u);
		s.total = a.count;
		s.pad = 0;
		s.first = i;
		out[atomicAdd(&ctr->pairs, 1ull)] = s;
	}
}

__device__ __forceinline__ uint32_t super_byte(const uint8_t *__restrict__ reads, const Piece &p, uint32_t k)
{
	return p.rev ? linkk::link_complement(reads[p.src - k]) : reads[p.src + k];
}

// The slices of *.supertig.gap.data: one wavefront per piece.  A piece's destination begins on a 64-byte boundary unless it is the
// first of its slice; bytes up to the first 4-byte boundary and behind the last one go out one per lane, the rest as one dword
// per lane, 256 consecutive bytes per wavefront store.  The source bytes are consecutive addresses too, ascending or (rev)
// descending through the complement table (rev_com_seq, seqKmer.cpp:83-91).  The host has checked every piece against its read.
// A source has no alignment in common with its destination and may run backwards, so a lane fetches the four bytes of its dword
// one by one (four byte loads per lane, each of them 64 consecutive addresses per wavefront) and not as one dword: the stores are
// full-width, the loads are not.  What that costs has not been measured.
__global__ __launch_bounds__(kSuperThreads) void k_super_slices(const Piece *__restrict__ pieces, uint64_t n_pieces, const uint8_t *__restrict__ reads,
                                                                uint8_t *__restrict__ out)
{
	const uint32_t lane = threadIdx.x & (kWave - 1);
	const uint64_t wave = ((uint64_t)blockIdx.x * kSuperThreads + threadIdx.x) / kWave;
	const uint64_t n_waves = (uint64_t)gridDim.x * (kSuperThreads / kWave);
	for (uint64_t w = wave; w < n_pieces; w += n_waves) {
		const Piece p = pieces[w];
		uint32_t head = (uint32_t)(-(int64_t)p.dst & 3);
		if (head > p.len) head = p.len;
		const uint32_t words = (p.len - head) / 4, tail = p.len - head - 4 * words;
		if (lane < head) out[p.dst + lane] = (uint8_t)super_byte(reads, p, lane);
		for (uint32_t j = lane; j < words; j += kWave) {
			const uint32_t k = head + 4 * j;
			const uint32_t v = super_byte(reads, p, k) | (super_byte(reads, p, k + 1) << 8) | (super_byte(reads, p, k + 2) << 16) |
			                   (super_byte(reads, p, k + 3) << 24);
			*reinterpret_cast<uint32_t *>(out + p.dst + k) = v;
		}
		if (lane < tail) out[p.dst + head + 4 * words + lane] = (uint8_t)super_byte(reads, p, head + 4 * words + lane);
	}
}

} // namespace superk
