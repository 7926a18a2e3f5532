// dbgk_clean.h -- CLEAN: clean_adapter / clean_lowqual of the clean_illumina module on the GPU (gfx950 only).
//
// Reference semantics (files of the reference's clean_illumina/ directory):
//   local_ungapped_aligning   clean_adapter.cpp:94-157   cell = max(0, up-left cell + pair score), first maximum in row-major order,
//                                                        start found by walking up-left to a cell of score 0
//   thread_trimReads          clean_adapter.cpp:174-231  adapters in file order, the first one that reaches the cutoff wins
//   thread_cleanlowqual       clean_lowqual.cpp:65-188   error sum of the read, break points, the first longest block
//
// k_clean_adapter keeps no matrix: a cell depends on its up-left neighbour alone, so every diagonal is a running sum that restarts
// behind a cell where it falls to <= 0.  One read per wave, one diagonal per lane, the adapter position as the wave-uniform loop
// counter; the lanes' best cells are reduced on the key (-score, read_end, adapter_end), which is the row-major order of the
// reference's strict `>` scan.  Reads of up to kCleanSlice bases are coded once into LDS beside the adapter codes; longer reads, and
// every read when the adapter set exceeds kCleanAdapterBytes, take the same code out of global memory.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dbgk {
namespace cleank {

constexpr int kCleanWaves = 4;                    // reads per workgroup
constexpr uint32_t kCleanSlice = 1024;            // longest read that is aligned out of LDS
constexpr uint32_t kCleanSliceBytes = kCleanSlice + 16; // whole dwords from the one below the first byte, and a sentinel behind the last
constexpr uint32_t kCleanAdapterBytes = 4096;     // largest adapter set (all codes back to back) that is held in LDS
constexpr int kLowqualThreads = 256;              // reads per workgroup of k_clean_lowqual
constexpr uint32_t kLowqualChunk = 8192;          // bytes of bases (and of qualities) staged at a time

struct AdapterHit { // == dbgk_adapter_hit
	int32_t adapter, score, read_start, read_end, adapter_start, adapter_end;
};

struct LowqualBlock { // == dbgk_lowqual_block
	double error_sum;
	int32_t start, length, trimmed, reserved;
};

// device counters of one batch
struct CleanCounters {
	unsigned long long by_lds, by_global, hits, cells;
	unsigned int n_long, pad;
};

// alphabet[] of clean_adapter.cpp:54-64 (bytes from 128 on, an out-of-bounds read there, count as 4 too).  The host codes the
// adapters the same way but with 5 for everything else, so that "equal codes" alone is the +1 of scoreMatrix: N never matches N.
constexpr uint32_t kReadOther = 4u, kAdapterOther = 5u;

__host__ __device__ __forceinline__ uint32_t clean_code(uint32_t c)
{
	const uint32_t u = c & 0xDFu;
	const bool letter = c < 128u && (u == 0x41u || u == 0x43u || u == 0x47u || u == 0x54u);
	return letter ? ((c >> 1) ^ (c >> 2)) & 3u : kReadOther;
}

// the read of a wave as codes; positions outside [0, L) give kReadOther, which equals no adapter code
struct LdsCodes { // p[L] holds kReadOther
	const uint8_t *p;
	uint32_t L;
	__device__ __forceinline__ uint32_t at(int32_t i) const { return p[min((uint32_t)i, L)]; }
};
struct GlobalCodes {
	const uint8_t *p;
	uint32_t L;
	__device__ __forceinline__ uint32_t at(int32_t i) const { return (uint32_t)i < L ? clean_code(p[i]) : kReadOther; }
};

__device__ __forceinline__ int32_t wave_max_i32(int32_t v)
{
	for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
	return v;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
	for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int32_t)v, off, 64));
	return v;
}

// local_ungapped_aligning of one read against one adapter (L, A >= 1): true when the best score reaches the cutoff, `h` then holds
// the reference's numbers (1-based, inclusive).  The whole wave calls it and gets the same answer in every lane.
template <class R>
__device__ bool clean_align(const R &rd, int32_t L, const uint8_t *__restrict__ ad, int32_t A, int32_t cutoff, AdapterHit &h)
{
	const int32_t lane = (int32_t)(threadIdx.x & 63u);
	// best cell of the diagonals this lane has walked: score, 0-based end and start in the read, the diagonal d = i - j
	int32_t bs = 0, be = 0, bst = 0, bd = 0;
	const int32_t n_diag = L + A - 1;
	for (int32_t r0 = 0; r0 < n_diag; r0 += 64) {
		const int32_t d_lo = r0 - (A - 1), d = d_lo + lane;
		// adapter positions at which some lane of this round is inside the read
		const int32_t j_lo = max(0, -(d_lo + 63)), j_hi = min(A - 1, L - 1 - d_lo);
		int32_t s = 0, st = max(d, 0), rs = 0, re = 0, rst = 0;
		for (int32_t j = j_lo; j <= j_hi; ++j) {
			const uint32_t a = ad[j];
			const int32_t i = d + j;
			s += rd.at(i) == a ? 1 : -2;
			if (s <= 0) { // the run ends; the next one starts behind this cell
				s = 0;
				st = i + 1;
			} else if (s > rs) { // the first cell where the diagonal reaches its maximum
				rs = s;
				re = i;
				rst = st;
			}
		}
		// smallest (-score, read_end, adapter_end); on one read_end the smaller adapter_end is the larger d
		if (rs > bs || (rs == bs && rs > 0 && (re < be || (re == be && d > bd)))) {
			bs = rs;
			be = re;
			bst = rst;
			bd = d;
		}
	}
	const int32_t best = wave_max_i32(bs);
	if (best < cutoff) return false; // the cutoff is >= 1: a wave without any positive cell ends here too
	const uint32_t end = wave_min_u32(bs == best ? (uint32_t)be : 0xFFFFFFFFu);
	const bool tie = bs == best && (uint32_t)be == end;
	const int32_t diag = wave_max_i32(tie ? bd : INT32_MIN);
	const int src = __ffsll((long long)__ballot(tie && bd == diag)) - 1; // diagonals are distinct: exactly one lane
	const int32_t start = __shfl(bst, src, 64);
	h.score = best;
	h.read_start = start + 1;
	h.read_end = (int32_t)end + 1;
	h.adapter_start = start - diag + 1;
	h.adapter_end = (int32_t)end - diag + 1;
	return true;
}

// the adapters in the order they are tried; the first one that reaches the cutoff is the hit (clean_adapter.cpp:189-206)
template <class R>
__device__ void clean_one(const R &rd, int32_t L, const uint8_t *__restrict__ ad, const uint32_t *__restrict__ ad_off, uint32_t n_ad,
                          int32_t cutoff, AdapterHit *__restrict__ out, unsigned long long &cells, unsigned long long &found)
{
	AdapterHit h{-1, 0, 0, 0, 0, 0};
	for (uint32_t a = 0; a < n_ad; ++a) {
		const uint32_t ao = ad_off[a];
		const int32_t A = (int32_t)(ad_off[a + 1] - ao);
		if (L < 1 || A < 1) continue;
		cells += (unsigned long long)L * (unsigned long long)A;
		if (clean_align(rd, L, ad + ao, A, cutoff, h)) {
			h.adapter = (int32_t)a;
			found++;
			break;
		}
	}
	if ((threadIdx.x & 63u) == 0u) *out = h;
}

// GLOBAL = false: every read of the batch, one per wave, coded into LDS; reads longer than kCleanSlice are appended to long_list.
// GLOBAL = true : reads and adapter codes out of global memory: the listed reads (use_list) or, for an adapter set that does not
//                 fit the LDS form, every read of the batch.
template <bool GLOBAL>
__global__ __launch_bounds__(kCleanWaves * 64) void k_clean_adapter(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ off, uint32_t n_reads,
                                                                    const uint8_t *__restrict__ ad_codes, const uint32_t *__restrict__ ad_off,
                                                                    uint32_t n_ad, int32_t cutoff, uint32_t use_list,
                                                                    AdapterHit *__restrict__ hits, uint32_t *__restrict__ long_list,
                                                                    CleanCounters *__restrict__ ctr)
{
	__shared__ __attribute__((aligned(16))) uint8_t lds_read[GLOBAL ? 16 : kCleanWaves * kCleanSliceBytes];
	__shared__ __attribute__((aligned(16))) uint8_t lds_ad[GLOBAL ? 16 : kCleanAdapterBytes];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (!GLOBAL) { // the adapter codes (at most kCleanAdapterBytes, the host's choice of form; the buffer is padded to whole dwords)
		const uint32_t n_dw = (ad_off[n_ad] + 3u) >> 2;
		for (uint32_t w = threadIdx.x; w < n_dw; w += kCleanWaves * 64)
			reinterpret_cast<uint32_t *>(lds_ad)[w] = reinterpret_cast<const uint32_t *>(ad_codes)[w];
		__syncthreads();
	}
	const uint32_t n_items = (GLOBAL && use_list) ? ctr->n_long : n_reads;
	unsigned long long cells = 0, done = 0, found = 0;
	for (uint64_t item = (uint64_t)blockIdx.x * kCleanWaves + wave; item < n_items; item += (uint64_t)gridDim.x * kCleanWaves) {
		const uint32_t r = (GLOBAL && use_list) ? long_list[item] : (uint32_t)item;
		const uint64_t o = off[r];
		const uint64_t len64 = off[r + 1] - o;
		const int32_t L = (int32_t)len64; // < 2^30, checked by the host
		if (GLOBAL) {
			clean_one(GlobalCodes{seq + o, (uint32_t)L}, L, ad_codes, ad_off, n_ad, cutoff, hits + r, cells, found);
			done++;
		} else {
			if (len64 > kCleanSlice) {
				if (lane == 0) long_list[atomicAdd(&ctr->n_long, 1u)] = r;
				continue;
			}
			uint8_t *slice = lds_read + wave * kCleanSliceBytes;
			// whole dwords from the one that holds the first byte through the one that holds position L, which gets the sentinel
			// (the batch buffer has 16 spare bytes); bytes behind the read are coded as kReadOther
			const uint64_t a0 = o & ~3ull;
			const uint32_t shift = (uint32_t)(o - a0), stop = shift + (uint32_t)L, n_dw = (stop >> 2) + 1u;
			for (uint32_t w = lane; w < n_dw; w += 64u) {
				const uint32_t v = *reinterpret_cast<const uint32_t *>(seq + a0 + 4ull * w);
				uint32_t codes = 0;
#pragma unroll
				for (uint32_t b = 0; b < 4; ++b) {
					const uint32_t c = 4u * w + b < stop ? clean_code((v >> (8u * b)) & 0xFFu) : kReadOther;
					codes |= c << (8u * b);
				}
				reinterpret_cast<uint32_t *>(slice)[w] = codes;
			}
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			clean_one(LdsCodes{slice + shift, (uint32_t)L}, L, lds_ad, ad_off, n_ad, cutoff, hits + r, cells, found);
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			done++;
		}
	}
	if (lane == 0) {
		if (done) atomicAdd(GLOBAL ? &ctr->by_global : &ctr->by_lds, done);
		if (found) atomicAdd(&ctr->hits, found);
		if (cells) atomicAdd(&ctr->cells, cells);
	}
}

// thread_cleanlowqual (clean_lowqual.cpp:84-160) for reads whose base and quality strings have equal lengths: one read per lane,
// the bytes of the workgroup's reads staged through LDS in chunks so that the global loads are coalesced.  The doubles are the
// reference's bit for bit: one lane adds one read's table values in read order, the cutoff test is a plain multiply followed by a
// compare, and floating-point contraction is switched off for this kernel so that no multiply is ever fused into an add.
__global__ __launch_bounds__(kLowqualThreads) void k_clean_lowqual(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual,
                                                                   const uint64_t *__restrict__ off, uint32_t n_reads,
                                                                   const double *__restrict__ table, double cutoff, uint32_t shift,
                                                                   LowqualBlock *__restrict__ out)
{
#pragma clang fp contract(off)
	__shared__ double tab[256];
	__shared__ __attribute__((aligned(16))) uint8_t lds_b[kLowqualChunk], lds_q[kLowqualChunk];
	const uint32_t tid = threadIdx.x;
	tab[tid] = table[tid];
	const uint64_t r0 = (uint64_t)blockIdx.x * kLowqualThreads;
	const uint64_t r = r0 + tid;
	const bool active = r < n_reads;
	const uint64_t lo = active ? off[r] : 0ull, hi = active ? off[r + 1] : 0ull;
	const uint64_t g_lo = off[r0], g_hi = off[min(r0 + (uint64_t)kLowqualThreads, (uint64_t)n_reads)];
	double sum = 0.0, accum_error = 0.0;
	int32_t accum_length = 0, last = 0, max_start = 0, max_len = 0;
	for (uint64_t c0 = g_lo & ~3ull; c0 < g_hi; c0 += kLowqualChunk) {
		__syncthreads(); // the chunk before has been consumed (first round: tab[] is complete)
		const uint32_t n_dw = (uint32_t)((min((uint64_t)kLowqualChunk, g_hi - c0) + 3ull) >> 2); // (both buffers have 16 spare bytes)
		for (uint32_t w = tid; w < n_dw; w += kLowqualThreads) {
			reinterpret_cast<uint32_t *>(lds_b)[w] = *reinterpret_cast<const uint32_t *>(seq + c0 + 4ull * w);
			reinterpret_cast<uint32_t *>(lds_q)[w] = *reinterpret_cast<const uint32_t *>(qual + c0 + 4ull * w);
		}
		__syncthreads();
		const uint64_t p0 = max(lo, c0), p1 = min(hi, c0 + kLowqualChunk);
		for (uint64_t p = p0; p < p1; ++p) {
			const uint32_t at = (uint32_t)(p - c0);
			const uint32_t q = lds_b[at] == 'N' ? (shift & 0xFFu) : lds_q[at]; // an upper-case N takes the quality 0 (:90-93)
			const double e = tab[q];
			sum += e;
			accum_error += e;
			accum_length++;
			if (accum_error > cutoff * (double)accum_length) { // a break point (:120-135): the block in front of it is a candidate
				const int32_t j = (int32_t)(p - lo);
				if (j - last > max_len) {
					max_len = j - last;
					max_start = last + 1;
				}
				accum_error = 0.0;
				accum_length = 0;
				last = j + 1;
			}
		}
	}
	if (!active) return;
	const int32_t n = (int32_t)(hi - lo); // < 2^30, checked by the host
	if (n - last > max_len) { // the tail behind the last break point (:139-148)
		max_len = n - last;
		max_start = last + 1;
	}
	LowqualBlock b;
	b.error_sum = sum;
	b.trimmed = sum > cutoff * (double)n ? 1 : 0;
	b.reserved = 0;
	if (b.trimmed) {
		const bool kept = max_start >= 1 && max_start <= n;
		b.start = kept ? max_start : 0;
		b.length = kept ? max_len : 0;
	} else {
		b.start = n ? 1 : 0;
		b.length = n;
	}
	out[r] = b;
}

} // namespace cleank
} // namespace dbgk
