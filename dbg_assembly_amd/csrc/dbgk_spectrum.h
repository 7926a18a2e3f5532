// SPECTRUM: the two table scans of the correct_error module that choose k and the low-frequency cutoff.
//
// k_kf_spectrum   histogram of the byte counters of a finalized KFREQ table (what the original kmerfreq prints as
//                 <lib>.kmer.freq.stat): bins 1..255, bin 0 is left to the host (n minus the other bins).
// k_mut_scan      simulate_lowfreq_kmer (correct_error/simulate_lowfreq_kmer.cpp:71-119): every `skip` bases of a
//                 sequence one base is mutated and the k windows over it are looked up in the loaded 1-bit table
//                 (marked on both strands, so the lookup is on the forward value); hist[absent windows]++.
//
// Both are memory scans whose loops depend on the sizes alone, never on what the table or the sequences hold.
#pragma once

namespace spec {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCopies = 8;          // LDS copies of the histogram per wave: lanes l and l + 8 share one
constexpr int kInFlight = 4;        // 16-byte loads a lane has in flight
constexpr int kMaxK = 19;           // dbgk_corr_create's limit

// One non-zero counter byte into the lane's copy.  A word is [bin][copy]: the 8 copies of one bin fill 8 banks.
__device__ __forceinline__ void count_byte(uint32_t *h, uint32_t c)
{
	if (c) atomicAdd(&h[c * kCopies], 1u);
}

__device__ __forceinline__ void count_word(uint32_t *h, uint32_t w)
{
	if (w == 0u) return;
	count_byte(h, w & 0xFFu);
	count_byte(h, (w >> 8) & 0xFFu);
	count_byte(h, (w >> 16) & 0xFFu);
	count_byte(h, w >> 24);
}

// bins[c] += number of i in [first, first + n) with counts[i] == c, for c = 1..255.  `counts` is 16-byte aligned.
// The range is cut into head bytes up to the first multiple of 16, whole 16-byte quads, and tail bytes; head and tail
// are at most 15 bytes each and belong to workgroup 0.  A workgroup adds fewer than 2^32 bytes (the host sizes the grid).
__global__ __launch_bounds__(kThreads) void k_kf_spectrum(const uint8_t *__restrict__ counts, uint64_t first, uint64_t n,
                                                           unsigned long long *__restrict__ bins)
{
	__shared__ uint32_t lds[kWaves * 256 * kCopies];
	for (int i = threadIdx.x; i < kWaves * 256 * kCopies; i += kThreads) lds[i] = 0;
	__syncthreads();
	uint32_t *h = lds + (threadIdx.x / 64) * (256 * kCopies) + (threadIdx.x & (kCopies - 1));

	const uint64_t end = first + n;
	const uint64_t head_end = min((first + 15ull) & ~15ull, end);
	const uint64_t body_end = max(end & ~15ull, head_end);
	if (blockIdx.x == 0) {
		const uint32_t t = threadIdx.x & 15u;
		if (threadIdx.x < 16) {
			if (first + t < head_end) count_byte(h, counts[first + t]);
		} else if (threadIdx.x < 32) {
			if (body_end + t < end) count_byte(h, counts[body_end + t]);
		}
	}
	const uint64_t q0 = head_end >> 4, nq = (body_end - head_end) >> 4;
	const uint4 *__restrict__ quads = reinterpret_cast<const uint4 *>(counts) + q0;
	const uint64_t stride = (uint64_t)gridDim.x * kThreads;
	for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < nq; i += stride * kInFlight) {
		uint4 v[kInFlight];
#pragma unroll
		for (int j = 0; j < kInFlight; ++j) {
			const uint64_t q = i + (uint64_t)j * stride;
			v[j] = q < nq ? quads[q] : make_uint4(0u, 0u, 0u, 0u);
		}
#pragma unroll
		for (int j = 0; j < kInFlight; ++j) {
			if ((v[j].x | v[j].y | v[j].z | v[j].w) == 0u) continue; // nearly every quad: no LDS traffic
			count_word(h, v[j].x);
			count_word(h, v[j].y);
			count_word(h, v[j].z);
			count_word(h, v[j].w);
		}
	}
	__syncthreads();
	// thread c owns bin c: its copies in every wave, flushed once
	unsigned long long sum = 0;
	const uint32_t c = threadIdx.x;
#pragma unroll
	for (int w = 0; w < kWaves; ++w)
#pragma unroll
		for (int j = 0; j < kCopies; ++j) sum += lds[w * (256 * kCopies) + c * kCopies + j];
	if (c != 0u && sum) atomicAdd(&bins[c], sum);
}

// the module's alphabet (correct_error/seqKmer.cpp): ACGT = 0..3 in either case, N and n = 0; any other byte reads as A
__device__ __forceinline__ uint32_t code_of(uint8_t b)
{
	const uint32_t u = b & 0xDFu; // upper case
	return (u == 'C' ? 1u : 0u) + (u == 'G' ? 2u : 0u) + (u == 'T' ? 3u : 0u);
}

// bit v of the loaded table (dbgk_correct.h: bit 7 - v % 8 of byte v / 8), v < 4^k
__device__ __forceinline__ uint32_t table_bit(const uint32_t *__restrict__ tab, uint64_t v)
{
	return (tab[v >> 5] >> corr::bit_in_word(v)) & 1u;
}

// One site per lane.  Site g of all `n_sites` belongs to the sequence s with site_lo[s] <= g < site_lo[s + 1] (found in
// `steps` halvings, a number the host derives from n_seqs) and starts at base (g - site_lo[s]) * skip of it: the
// fragment of 2k - 1 bases lies inside the sequence because the host counts a sequence's sites that way.
__global__ __launch_bounds__(kThreads) void k_mut_scan(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ off,
                                                        const uint64_t *__restrict__ site_lo, uint64_t n_seqs, uint32_t steps,
                                                        uint64_t n_sites, uint32_t skip, int k, const uint32_t *__restrict__ tab,
                                                        uint64_t total, unsigned long long *__restrict__ hist)
{
	__shared__ unsigned long long bins[32];
	if (threadIdx.x < 32) bins[threadIdx.x] = 0;
	__syncthreads();
	const int lane = corr::lane_id();
	const uint64_t mask = total - 1;
	const uint64_t stride = (uint64_t)gridDim.x * kThreads;
	const uint64_t rounds = (n_sites + stride - 1) / stride;
	unsigned long long mine = 0; // lane b collects bin b of its wave
	for (uint64_t r = 0; r < rounds; ++r) {
		const uint64_t g = r * stride + (uint64_t)blockIdx.x * kThreads + threadIdx.x;
		const bool live = g < n_sites;
		uint32_t absent = 0;
		if (live) {
			uint64_t lo = 0, len = n_seqs; // the last s in [0, n_seqs) with site_lo[s] <= g
			for (uint32_t t = 0; t < steps; ++t) {
				const uint64_t half = len >> 1;
				const uint64_t mid = lo + half;
				const bool right = half != 0 && site_lo[mid] <= g;
				lo = right ? mid : lo;
				len = right ? len - half : half;
			}
			const uint8_t *p = seq + off[lo] + (g - site_lo[lo]) * (uint64_t)skip;
			uint64_t v = 0;
			for (int j = 0; j < k - 1; ++j) v = (v << 2) | code_of(p[j]);
			v = (v << 2) | ((code_of(p[k - 1]) + 1u) & 3u);
			uint32_t present = table_bit(tab, v & mask);
#pragma unroll
			for (int j = 1; j < kMaxK; ++j) {
				if (j < k) {
					v = ((v << 2) | code_of(p[k - 1 + j])) & mask;
					present += table_bit(tab, v);
				}
			}
			absent = (uint32_t)k - present;
		}
		for (int b = 0; b <= k; ++b) {
			const unsigned long long c = (unsigned long long)__popcll(corr::ballot(live && absent == (uint32_t)b));
			if (lane == b) mine += c;
		}
	}
	if (lane <= k && mine) atomicAdd(&bins[lane], mine);
	__syncthreads();
	if ((int)threadIdx.x <= k && bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
}

} // namespace spec
