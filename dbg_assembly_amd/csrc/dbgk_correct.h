// CORRECT: correct_error_reads (correct_error/correct.cpp:146-335 and the trees of :380-635) on the GPU.
//
// The table is the LOADED 1-bit table (after the loader's mirror), bytes in the reference's order: bit v is
// bit 7 - v % 8 of byte v / 8; kernels read it as little-endian 32-bit words.  Every lookup is on the
// forward k-mer value exactly as seq2bit (correct_error/seqKmer.cpp:52-60) forms it, code 4 included; a value
// at or beyond 4^k (where the reference reads out of bounds) counts as low.
//
// Kernels: k_corr_classify (all reads; finishes those whose k-mers are all high), k_corr_fix (one wave per read
// of the work list, read + mask + tree frontier in LDS) and k_corr_overflow (the same code with everything in a
// per-wave slice of global memory, for reads whose frontier or length does not fit in LDS).
//
// A tree node is (last k-1 bases, change count, <= 2 edits): a path holds at most min(2, -c) edits
// (correct.cpp:387-390), a correction is applied only when exactly one frontier node has the minimum change,
// and the node COUNT (not the nodes) decides when a cycle is discarded -- so no node array is needed.
#pragma once

namespace corr {

constexpr int kWave = 64;
constexpr int kLdsNodes = 256;     // frontier capacity per buffer in LDS (two buffers)
constexpr int kLdsReadLen = 1024;  // longer reads go to the overflow kernel
constexpr int kLdsMaskWords = kLdsReadLen / 64 + 1;

struct CorrParams {
	int k, m, c, x, n, r;
	uint64_t total; // 4^k
};

struct TNode {
	uint64_t ctx;  // rightward: last k-1 bases; leftward: first k-1 bases of the path, nearest base highest
	uint64_t info; // change [0,2) | base0 [2,4) | base1 [4,6) | pos0 [6,35) | pos1 [35,64)   (positions 1-based)
};

// per-read working set: LDS in k_corr_fix, global memory in k_corr_overflow
struct Work {
	uint8_t *read;
	uint64_t *mask;
	TNode *fa, *fb;
	uint32_t cap;
};

__device__ __forceinline__ uint32_t base_code(uint8_t b)
{
	switch (b) {
		case 'A': case 'a': case 'N': case 'n': return 0;
		case 'C': case 'c': return 1;
		case 'G': case 'g': return 2;
		case 'T': case 't': return 3;
		default: return 4;
	}
}

__device__ __forceinline__ uint8_t base_char(uint32_t j) { return (uint8_t)(j == 0 ? 'A' : j == 1 ? 'C' : j == 2 ? 'G' : 'T'); }

__device__ __forceinline__ bool is_high(const uint32_t *__restrict__ tab, uint64_t v, uint64_t total)
{
	if (v >= total) return false;
	const uint32_t w = tab[v >> 5];
	return (w >> ((((uint32_t)(v >> 3) & 3u) << 3) + 7u - ((uint32_t)v & 7u))) & 1u;
}

__device__ __forceinline__ uint32_t bit_in_word(uint64_t v) { return ((((uint32_t)(v >> 3) & 3u) << 3) + 7u - ((uint32_t)v & 7u)); }

// seq2bit of n bytes from p, byte `sub_at` replaced by `sub` (sub_at < 0: none)
__device__ __forceinline__ uint64_t seq2bit(const uint8_t *p, int n, int sub_at = -1, uint8_t sub = 0)
{
	uint64_t v = 0;
	for (int i = 0; i < n; ++i) v = (v << 2) | base_code(i == sub_at ? sub : p[i]);
	return v;
}

__device__ __forceinline__ uint64_t revcomp(uint64_t v, int k)
{
	v = ~v;
	v = ((v & 0x3333333333333333ull) << 2) | ((v & 0xCCCCCCCCCCCCCCCCull) >> 2);
	v = ((v & 0x0F0F0F0F0F0F0F0Full) << 4) | ((v & 0xF0F0F0F0F0F0F0F0ull) >> 4);
	v = ((v & 0x00FF00FF00FF00FFull) << 8) | ((v & 0xFF00FF00FF00FF00ull) >> 8);
	v = ((v & 0x0000FFFF0000FFFFull) << 16) | ((v & 0xFFFF0000FFFF0000ull) >> 16);
	v = (v << 32) | (v >> 32);
	return v >> (64 - 2 * k);
}

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }

__device__ __forceinline__ int get_bit(const uint64_t *mask, int i) { return (int)((mask[i >> 6] >> (i & 63)) & 1ull); }

// first index >= i whose mask bit equals want, or nk
__device__ __forceinline__ int next_bit(const uint64_t *mask, int i, int nk, int want)
{
	while (i < nk) {
		uint64_t w = mask[i >> 6];
		if (!want) w = ~w;
		w >>= (i & 63);
		if (w) {
			const int j = i + __builtin_ctzll(w);
			return j < nk ? j : nk;
		}
		i = (i | 63) + 1;
	}
	return nk;
}

// ---- the high/low mask of the read as it stands (get_cont_kmerfreq_region, correct.cpp:16-69) ----------------------
__device__ void scan_mask(const Work &w, int L, const CorrParams &P, const uint32_t *__restrict__ tab)
{
	const int nk = L - P.k + 1, lane = lane_id();
	for (int base = 0; base < nk; base += kWave) {
		const int p = base + lane;
		const bool h = p < nk && is_high(tab, seq2bit(w.read + p, P.k), P.total);
		const uint64_t b = ballot(h);
		if (lane == 0) w.mask[base >> 6] = b;
	}
	__syncthreads();
}

// ---- correct_one_base (correct.cpp:74-107): k windows [s, s + k) all high after one substitution at s + k - 1 -------
__device__ bool one_base_fix(const Work &w, int s, const CorrParams &P, const uint32_t *__restrict__ tab)
{
	const int k = P.k, lane = lane_id(), e = s + k - 1; // 0-based position of the error base
	const uint8_t err = w.read[e];
	uint32_t fails = 0;
	for (int c0 = 0; c0 < 4 * k; c0 += kWave) {
		const int c = c0 + lane;
		const bool valid = c < 4 * k;
		const int b = valid ? c / k : 0, j = s + (valid ? c % k : 0);
		const bool low = valid && !is_high(tab, seq2bit(w.read + j, k, e - j, base_char(b)), P.total);
		for (int bb = 0; bb < 4; ++bb)
			if (ballot(low && b == bb)) fails |= 1u << bb;
	}
	for (int b = 0; b < 4; ++b) {
		if (base_char(b) == err || (fails >> b) & 1u) continue;
		__syncthreads();
		if (lane == 0) w.read[e] = base_char(b);
		__syncthreads();
		return true;
	}
	return false;
}

struct TreeResult {
	int corrected; // num_corrected
	int trim;      // len_need_trim
};

// ---- correct_multi_bases_rightward / _leftward (correct.cpp:380-485, 514-615) on a frontier of TNode -----------------
// start / end: 1-based read positions (check_start, check_end).  *overflow: the frontier outgrew w.cap (the read
// is abandoned; nothing of it has been written outside the working set).
__device__ TreeResult bb_tree(const Work &w, int L, const CorrParams &P, const uint32_t *__restrict__ tab, int start,
                              int end, bool right, bool modify, int max_change, int *last_pos, uint32_t *hits, bool *overflow)
{
	const int k = P.k, lane = lane_id();
	const uint64_t km1 = (k > 1) ? ((1ull << (2 * (k - 1))) - 1) : 0ull;
	const uint64_t full = (1ull << (2 * k)) - 1;
	if (max_change > 2) max_change = 2;
	uint64_t sbits = 0, root = 0;
	if (right) root = seq2bit(w.read + (start - k), k - 1) & km1;
	else sbits = seq2bit(w.read + start, k - 1);
	TNode *A = w.fa, *B = w.fb;
	__syncthreads();
	if (lane == 0) { A[0].ctx = root; A[0].info = 0; }
	__syncthreads();
	uint32_t F = 1;
	uint64_t nodes = 0;
	int cyc = start, depth = 0;
	const int step = right ? 1 : -1;
	while (right ? cyc <= end : cyc >= end) {
		const uint8_t here = w.read[cyc - 1];
		const uint64_t sb = depth < k - 1 ? (sbits >> (2 * depth)) : 0ull;
		uint32_t cnt = 0;
		for (uint32_t c0 = 0; c0 < 4 * F; c0 += kWave) {
			const uint32_t c = c0 + lane;
			const bool valid = c < 4 * F;
			const uint32_t j = c & 3;
			TNode nd = valid ? A[c >> 2] : TNode{0, 0};
			uint64_t km, nctx;
			if (right) {
				km = ((nd.ctx << 2) | j) & full;
				nctx = km & km1;
			} else {
				km = ((uint64_t)j << (2 * (k - 1))) | nd.ctx | sb;
				nctx = k > 1 ? ((((uint64_t)j << (2 * (k - 2))) | (nd.ctx >> 2)) & km1) : 0ull;
			}
			const uint32_t ch = (uint32_t)(nd.info & 3u);
			const bool same = base_char(j) == here;
			const uint32_t nch = ch + (same ? 0u : 1u);
			const bool keep = valid && nch <= (uint32_t)max_change && is_high(tab, km, P.total);
			const uint64_t bal = ballot(keep);
			const uint32_t slot = cnt + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
			if (keep && slot < w.cap) {
				uint64_t info = (nd.info & ~3ull) | nch;
				if (!same) {
					if (ch == 0) info |= ((uint64_t)j << 2) | ((uint64_t)cyc << 6);
					else info |= ((uint64_t)j << 4) | ((uint64_t)cyc << 35);
				}
				B[slot].ctx = nctx;
				B[slot].info = info;
			}
			cnt += (uint32_t)__popcll(bal);
		}
		nodes += cnt;
		if (cnt >= 1 && nodes < (uint64_t)P.n) {
			if (cnt > w.cap) { *overflow = true; return {0, 0}; }
			__syncthreads();
			TNode *t = A; A = B; B = t;
			F = cnt;
		} else {
			if (nodes >= (uint64_t)P.n) *hits += 1;
			break;
		}
		cyc += step;
		++depth;
	}
	__syncthreads();
	// the minimum change and how many nodes carry it
	uint32_t count[3] = {0, 0, 0};
	for (uint32_t c0 = 0; c0 < F; c0 += kWave) {
		const uint32_t c = c0 + lane;
		const uint32_t ch = c < F ? (uint32_t)(A[c].info & 3u) : 3u;
		for (int v = 0; v < 3; ++v) count[v] += (uint32_t)__popcll(ballot(ch == (uint32_t)v));
	}
	const int mn = count[0] ? 0 : count[1] ? 1 : 2;
	const int trim = right ? end - cyc + 1 : cyc - end + 1;
	if (count[mn] != 1 || !(trim == 0 || modify)) return {0, trim};
	uint64_t info = 0;
	for (uint32_t c0 = 0; c0 < F; c0 += kWave) {
		const uint32_t c = c0 + lane;
		const bool hit = c < F && (int)(A[c].info & 3u) == mn;
		const uint64_t bal = ballot(hit);
		if (bal) { info = A[c0 + __builtin_ctzll(bal)].info; break; }
	}
	const int ne = (int)(info & 3u);
	const int p0 = (int)((info >> 6) & ((1u << 29) - 1)), p1 = (int)((info >> 35) & ((1u << 29) - 1));
	__syncthreads();
	if (lane == 0) {
		if (ne >= 1) w.read[p0 - 1] = base_char((uint32_t)(info >> 2) & 3u);
		if (ne >= 2) w.read[p1 - 1] = base_char((uint32_t)(info >> 4) & 3u);
	}
	__syncthreads();
	if (ne >= 1) {
		if (right && *last_pos == L + 1) *last_pos = ne == 2 ? max(p0, p1) : p0;
		if (!right && *last_pos == 0) *last_pos = ne == 2 ? min(p0, p1) : p0;
	}
	return {mn, trim};
}

// next high region of length >= m at or after kmer index i (0-based, [s, e)); s = nk when none
__device__ __forceinline__ void next_region(const uint64_t *mask, int i, int nk, int m, int *s, int *e)
{
	while (i < nk) {
		const int a = next_bit(mask, i, nk, 1);
		if (a >= nk) break;
		const int b = next_bit(mask, a, nk, 0);
		if (b - a >= m) { *s = a; *e = b; return; }
		i = b;
	}
	*s = *e = nk;
}

// ---- correct_one_read (correct.cpp:146-335) on the working set; returns false on frontier overflow ---------------
__device__ bool correct_read(const Work &w, int L, const CorrParams &P, const uint32_t *__restrict__ tab, dbgk_corr_rec &rec)
{
	const int k = P.k, nk = L - k + 1;
	int accum = 0;
	rec = dbgk_corr_rec{};
	rec.path = 1;
	if (nk <= 0) { rec.deleted = 1; return true; }
	scan_mask(w, L, P, tab);
	const int lane = lane_id();
	// one-base fix of interior low regions of exactly k k-mers
	for (int s = 0; s < nk;) {
		const int v = get_bit(w.mask, s);
		const int e = next_bit(w.mask, s, nk, !v);
		if (!v && s > 0 && e < nk) {
			if (accum >= P.c) break;
			if (e - s == k && one_base_fix(w, s, P, tab)) {
				rec.one_base++;
				accum++;
				if (lane == 0)
					for (int i = s; i < e; ++i) w.mask[i >> 6] |= 1ull << (i & 63);
				__syncthreads();
			}
		}
		s = e;
	}
	// high regions >= m k-mers, cut by m / 3 at inner edges, as 1-based inclusive k-mer indices
	const int cut = P.m / 3;
	int a, b;
	next_region(w.mask, 0, nk, P.m, &a, &b);
	if (a >= nk) { rec.deleted = 1; return true; }
	auto cut_start = [&](int s0) { return s0 + 1 != 1 ? s0 + 1 + cut : 1; };
	auto cut_end = [&](int e0) { return e0 != nk ? e0 - cut : e0; };
	int cs = cut_start(a), ce = cut_end(b); // current region
	int comb_start = cs, best_s = 0, best_e = 0, best_len = 0;
	bool overflow = false;
	for (;;) {
		int na, nb;
		next_region(w.mask, b, nk, P.m, &na, &nb);
		if (na >= nk) break;
		const int ns = cut_start(na), ne = cut_end(nb);
		bool fail;
		if (accum >= P.c) {
			fail = true;
		} else {
			int dummy = -1;
			TreeResult t = bb_tree(w, L, P, tab, ce + k, ns + k - 2, true, false, P.c - accum, &dummy, &rec.node_limit_hits, &overflow);
			if (overflow) return false;
			if (t.trim == 0 && t.corrected > 0) {
				rec.tree += t.corrected;
				accum += t.corrected;
				fail = false;
			} else {
				t = bb_tree(w, L, P, tab, ns - 1, ce + 1, false, false, P.c - accum, &dummy, &rec.node_limit_hits, &overflow);
				if (overflow) return false;
				fail = !(t.trim == 0 && t.corrected > 0);
				if (!fail) {
					rec.tree += t.corrected;
					accum += t.corrected;
				}
			}
		}
		if (fail) { // get_max_highFreq_region: close the combined region here
			if (ce - comb_start + 1 > best_len) { best_len = ce - comb_start + 1; best_s = comb_start; best_e = ce; }
			comb_start = ns;
		}
		a = na; b = nb; cs = ns; ce = ne;
	}
	if (ce - comb_start + 1 > best_len) { best_len = ce - comb_start + 1; best_s = comb_start; best_e = ce; }
	int lt = 0, rt = 0, llast = 0, rlast = L + 1;
	if (best_s > 1) {
		if (accum < P.c) {
			TreeResult t = bb_tree(w, L, P, tab, best_s - 1, 1, false, true, P.c - accum, &llast, &rec.node_limit_hits, &overflow);
			if (overflow) return false;
			lt = t.trim;
			if (t.corrected > 0) { rec.tree += t.corrected; accum += t.corrected; }
			else { lt = best_s - 1; llast = 0; }
		} else {
			lt = best_s - 1;
			llast = 0;
		}
	}
	const int he = best_e + k - 1;
	if (he < L) {
		if (accum < P.c) {
			TreeResult t = bb_tree(w, L, P, tab, he + 1, L, true, true, P.c - accum, &rlast, &rec.node_limit_hits, &overflow);
			if (overflow) return false;
			rt = t.trim;
			if (t.corrected > 0) { rec.tree += t.corrected; accum += t.corrected; }
			else { rt = L - he; rlast = L + 1; }
		} else {
			rt = L - he;
			rlast = L + 1;
		}
	}
	if (lt > 0 || (llast > 0 && llast <= P.x)) { lt += P.x; if (lt > L) lt = L; }
	if (rt > 0 || (rlast < L + 1 && rlast >= L - P.x + 1)) { rt += P.x; if (rt > L) rt = L; }
	rec.left_trim = (uint32_t)lt;
	rec.right_trim = (uint32_t)rt;
	rec.deleted = (L - lt - rt < P.r) ? 1 : 0;
	return true;
}

// ---- table construction ---------------------------------------------------------------------------------------------
// the loader's mirror (main_parallel_senior.cpp:310-329), in place: every set bit v with v <= rc(v) sets rc(v).  Bits
// added here have v >= rc(v), so they never act themselves (palindromes are already set): the result is an OR and
// does not depend on order.  *hifreq += number of such v (Kmer_hifreq_num).
__global__ void k_corr_seal(uint32_t *tab, uint64_t words, uint64_t total, int k, unsigned long long *hifreq)
{
	unsigned long long mine = 0;
	for (uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; wi < words; wi += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t w = __atomic_load_n(&tab[wi], __ATOMIC_RELAXED);
		while (w) {
			const uint32_t bit = (uint32_t)__builtin_ctz(w);
			w &= w - 1;
			const uint64_t v = wi * 32 + (bit >> 3) * 8 + (7 - (bit & 7));
			if (v >= total) continue;
			const uint64_t rc = revcomp(v, k);
			if (v <= rc) {
				atomicOr(&tab[rc >> 5], 1u << bit_in_word(rc));
				++mine;
			}
		}
	}
	if (mine) atomicAdd(hifreq, mine);
}

// the table kmerfreq -b 1 -m cutoff would write, after the loader: bit(v) = count[canonical(v)] > cutoff
__global__ void k_corr_from_counts(uint32_t *tab, uint64_t words, uint64_t total, int k, const uint8_t *__restrict__ counts,
                                   uint32_t cutoff, unsigned long long *hifreq)
{
	unsigned long long mine = 0;
	for (uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; wi < words; wi += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t out = 0;
		for (uint32_t t = 0; t < 32; ++t) {
			const uint64_t v = wi * 32 + t;
			if (v >= total) break;
			const uint64_t rc = revcomp(v, k);
			if (counts[v <= rc ? v : rc] > cutoff) {
				out |= 1u << bit_in_word(v);
				mine += v <= rc;
			}
		}
		tab[wi] = out;
	}
	if (mine) atomicAdd(hifreq, mine);
}

// ---- per-read kernels -----------------------------------------------------------------------------------------------
// all reads: a read whose k-mers are all high (or that has none) is finished here; the rest go to the work list
__global__ void k_corr_classify(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ off, uint32_t n_reads, CorrParams P,
                                const uint32_t *__restrict__ tab, uint8_t *__restrict__ out, dbgk_corr_rec *__restrict__ rec,
                                uint32_t *__restrict__ work, uint32_t *__restrict__ counters)
{
	const int lane = lane_id();
	const uint32_t waves = gridDim.x * (blockDim.x / kWave);
	for (uint32_t i = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave; i < n_reads; i += waves) {
		const uint64_t o = off[i];
		const int L = (int)(off[i + 1] - o), nk = L - P.k + 1;
		const uint8_t *r = seq + o;
		bool all = true;
		for (int base = 0; base < nk && all; base += 2 * kWave) { // two windows per lane in flight
			const int p0 = base + lane, p1 = base + kWave + lane;
			const bool l0 = p0 < nk && !is_high(tab, seq2bit(r + p0, P.k), P.total);
			const bool l1 = p1 < nk && !is_high(tab, seq2bit(r + p1, P.k), P.total);
			all = ballot(l0 || l1) == 0;
		}
		if (all) {
			for (int p = lane; p < L; p += kWave) out[o + p] = r[p];
			if (lane == 0) {
				dbgk_corr_rec q{};
				q.deleted = (nk < P.m || L < P.r) ? 1 : 0; // no k-mer / no region >= m / too short: correct.cpp:213-217,331
				rec[i] = q;
			}
		} else if (lane == 0) {
			work[atomicAdd(&counters[0], 1u)] = i;
		}
	}
}

__device__ __forceinline__ void finish(const Work &w, int L, uint8_t *out, const dbgk_corr_rec &q, dbgk_corr_rec *rec, uint32_t i)
{
	for (int p = lane_id(); p < L; p += kWave) out[p] = w.read[p];
	if (lane_id() == 0) rec[i] = q;
}

// one wave per read of the work list; read, mask and the two frontier buffers in LDS
__global__ __launch_bounds__(kWave) void k_corr_fix(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ off, CorrParams P,
                                                     const uint32_t *__restrict__ tab, uint8_t *__restrict__ out, dbgk_corr_rec *__restrict__ rec,
                                                     const uint32_t *__restrict__ work, uint32_t *__restrict__ ovf, uint32_t *__restrict__ counters)
{
	__shared__ TNode fa[kLdsNodes], fb[kLdsNodes];
	__shared__ uint64_t mask[kLdsMaskWords];
	__shared__ uint8_t rd[kLdsReadLen];
	const Work w{rd, mask, fa, fb, (uint32_t)kLdsNodes};
	const uint32_t n_work = counters[0];
	for (uint32_t t = blockIdx.x; t < n_work; t += gridDim.x) {
		const uint32_t i = work[t];
		const uint64_t o = off[i];
		const int L = (int)(off[i + 1] - o);
		bool ok = L <= kLdsReadLen;
		if (ok) {
			__syncthreads();
			for (int p = lane_id(); p < L; p += kWave) rd[p] = seq[o + p];
			__syncthreads();
			dbgk_corr_rec q;
			ok = correct_read(w, L, P, tab, q);
			if (ok) finish(w, L, out + o, q, rec, i);
		}
		if (!ok && lane_id() == 0) ovf[atomicAdd(&counters[1], 1u)] = i;
	}
}

// the reads k_corr_fix could not hold: the same code on a per-wave slice of global memory
__global__ __launch_bounds__(kWave) void k_corr_overflow(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ off, CorrParams P,
                                                          const uint32_t *__restrict__ tab, uint8_t *__restrict__ out,
                                                          dbgk_corr_rec *__restrict__ rec, const uint32_t *__restrict__ ovf, uint32_t n_ovf,
                                                          uint8_t *scratch, uint64_t slice_bytes, uint32_t max_len, uint32_t cap)
{
	uint8_t *base = scratch + (uint64_t)blockIdx.x * slice_bytes;
	const uint64_t mask_words = max_len / 64 + 1;
	TNode *fa = (TNode *)base;
	TNode *fb = fa + cap;
	uint64_t *mask = (uint64_t *)(fb + cap);
	uint8_t *rd = (uint8_t *)(mask + mask_words);
	const Work w{rd, mask, fa, fb, cap};
	for (uint32_t t = blockIdx.x; t < n_ovf; t += gridDim.x) {
		const uint32_t i = ovf[t];
		const uint64_t o = off[i];
		const int L = (int)(off[i + 1] - o);
		__syncthreads();
		for (int p = lane_id(); p < L; p += kWave) rd[p] = seq[o + p];
		__syncthreads();
		dbgk_corr_rec q;
		if (!correct_read(w, L, P, tab, q)) { // cap is sized so that this cannot happen; report it, do not guess
			q = dbgk_corr_rec{};
			q.path = 0xff;
		} else {
			q.path = 2;
		}
		finish(w, L, out + o, q, rec, i);
	}
}

} // namespace corr
