// DEFLATE stage (include/dbgk.h, GZ section; framing in dbgk_gz_frame.h; host side dbgk_host_gz.h; the rules are stated in DESIGN.md
// and restated in tests/deflate_restatement.py): bytes become BGZF-framed gzip members, one member per piece of kGzPiece bytes.
//
//   k_gz_members   ONE workgroup builds ONE member in its 64 KiB slot, from the piece staged in LDS:
//                    a lane takes kGzLaneBytes consecutive bytes: its CRC-32 state by table, brought to the end of the piece by a
//                    multiplication with x^(8 tail) mod P and XORed over the workgroup; the byte histogram by LDS atomics;
//                    level 2: matches, a chunk of 256 positions at a time -- every lane looks its 3-byte hash up in an LDS table that holds
//                    the last position of each hash in the chunks in front, then enters its own position with an LDS max; the second
//                    candidate is the position one back; both lengths are counted out of LDS; the greedy parse marks the positions
//                    on the path next[i] = i + max(1, len[i]) by pointer jumping, a ballot and a scan number them, the tokens go to
//                    the member's token array and their symbols into the two histograms;
//                    all lanes rank the used symbols by (count, symbol); lane 0 derives the code lengths, the canonical codes, the
//                    run-length coded length sequence and its own code, and composes the block header in LDS;
//                    a lane sums the bits of its slice, a scan over the workgroup places the slices;
//                    the slot's dwords are zeroed, and every lane composes its bits in a 64-bit register: a dword that is all its
//                    own is stored, the first and last one are ORed in, as are header, block header, end-of-block and trailer;
//                    a member whose dynamic block is not smaller than the stored one is written stored (level 0: always).
//                  The slot behind the last member takes the end marker.  Lane 0 reads the shader clock between the phases and adds
//                  the differences to three counters: the host divides the launch's time by them (dbgk_gz_timing).
//   (scan)         member sizes -> their offsets in the output (dbgk_sort.hip, rocPRIM)
//   k_gz_gather    a workgroup copies one member to its place: whole dwords of the output, funnel-shifted out of the slot's,
//                  and the up to three bytes in front of and behind them one by one
//
// No kernel waits for another workgroup.  Memory read: the text in whole 16-byte vectors up to n_bytes rounded up to 16; bytes at
// or behind n_bytes reach LDS and are used by nothing.
#pragma once

#define DBGK_GZ_HD __host__ __device__
#include "dbgk_gz_frame.h"
#include "dbgk_emit.h"

namespace dbgk {
namespace gzk {

using emitk::kWave;
using emitk::lane_id;
using gzf::kGzPiece;
using gzf::kGzSlot;

constexpr int kGzBlock = 256;
constexpr int kGzWaves = kGzBlock / kWave;
constexpr uint32_t kGzLaneBytes = kGzPiece / kGzBlock; // 255: the slice of a lane
static_assert(kGzLaneBytes * kGzBlock == kGzPiece && kGzPiece % 16 == 0, "a piece is 256 slices and starts at a 16-byte boundary");
constexpr int kGzLitSyms = 257;  // literals and end-of-block: level 1 uses no length symbol
constexpr int kGzLenSyms = 286;  // ... and the 29 length symbols of level 2
constexpr int kGzDistSyms = 30;
constexpr int kGzSeq = 320;      // room for 286 + 30 lengths
constexpr int kGzHashBits = 12;
constexpr uint32_t kGzMaxDist = 32768, kGzMaxMatch = 258, kGzMinMatch = 3;
constexpr uint32_t kGzFar = 4096; // a match of kGzMinMatch bytes farther back than this costs more than its literals: not used
constexpr int kGzClSyms = 19;
constexpr int kGzSymCap = 288;
constexpr int kGzHeadWords = 160; // block header: 17 + 19 * 3 + 316 * 14 bits at the most

// GC_CYC_*: shader-clock cycles that lane 0 of every workgroup saw between the phases of its members, summed: the share of each in
// the launch's time (dbgk_gz_timing)
enum Counter { GC_STORED = 0, GC_LITERALS, GC_MATCHES, GC_MATCH_BYTES, GC_CYC_MATCH, GC_CYC_HIST, GC_CYC_CODES, GC_CYC_ENCODE, GC_COUNT };

__constant__ uint8_t kGzClOrder[kGzClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct GzLds {
	uint8_t piece[kGzPiece];
	uint32_t crc_tab[256];
	uint32_t x8[16];              // x^(8 * 2^k) mod P
	uint32_t freq[kGzSymCap];
	uint32_t code[kGzSymCap];     // the code, first bit lowest | length << 16
	uint32_t sortf[kGzSymCap];    // the counts of the used symbols in rising order; then the array the lengths are derived in
	uint16_t sorts[kGzSymCap];    // ... and their symbols
	uint8_t len[kGzSymCap];       // literal / length code lengths
	uint32_t dfreq[32], dcode[32], dsortf[32]; // the distance code
	uint16_t dsorts[32];
	uint8_t dlen[32];
	uint8_t seq[kGzSeq];          // HLIT literal / length lengths, then HDIST distance lengths
	uint8_t cl_sym[kGzSeq + 6], cl_extra[kGzSeq + 6];
	uint32_t cl_freq[kGzClSyms], cl_code[kGzClSyms], cl_sortf[kGzClSyms];
	uint16_t cl_sorts[kGzClSyms];
	uint8_t cl_len[kGzClSyms + 1];
	uint32_t num[16], next[16];
	uint32_t head[kGzHeadWords];
	uint32_t wave_bits[kGzWaves], wave_crc[kGzWaves];
	uint32_t n_used, n_used_d, head_bits, hlit, hdist, n_seq;
	// level 2 only (a launch of another level does not ask for this part)
	struct Match {
		uint32_t htab[1 << kGzHashBits]; // position + 1 of the last occurrence of a 3-byte hash in the chunks in front; 0: none
		uint16_t jmp[kGzBlock];
		uint8_t sel[kGzBlock];
		uint32_t wave_cnt[kGzWaves];
		uint32_t entry, n_tok, n_match, match_bytes;
	} M;
};

// length 3..258 -> symbol, number and value of its extra bits
__device__ __forceinline__ void len_symbol(uint32_t len, uint32_t &sym, uint32_t &ebits, uint32_t &extra)
{
	const uint32_t l = len - 3u;
	if (l < 8u) { sym = 257u + l; ebits = 0; extra = 0; return; }
	if (l == 255u) { sym = 285u; ebits = 0; extra = 0; return; }
	ebits = 29u - (uint32_t)__clz((int)l); // floor(log2 l) - 2
	sym = 261u + 4u * ebits + ((l >> ebits) & 3u);
	extra = l & ((1u << ebits) - 1u);
}

// distance 1..32768 -> symbol, number and value of its extra bits
__device__ __forceinline__ void dist_symbol(uint32_t dist, uint32_t &sym, uint32_t &ebits, uint32_t &extra)
{
	const uint32_t d = dist - 1u;
	if (d < 4u) { sym = d; ebits = 0; extra = 0; return; }
	const uint32_t n = 31u - (uint32_t)__clz((int)d);
	ebits = n - 1u;
	sym = 2u * n + ((d >> ebits) & 1u);
	extra = d & ((1u << ebits) - 1u);
}

// a token: a literal byte, or bit 31 | (length - 3) << 15 | (distance - 1)
__device__ __forceinline__ uint32_t token_bits(const GzLds &L, uint32_t t)
{
	if (!(t >> 31)) return L.code[t] >> 16;
	uint32_t ls, le, lx, ds, de, dx;
	len_symbol(((t >> 15) & 0xFFu) + 3u, ls, le, lx);
	dist_symbol((t & 0x7FFFu) + 1u, ds, de, dx);
	return (L.code[ls] >> 16) + le + (L.dcode[ds] >> 16) + de;
}

__device__ __forceinline__ uint32_t bit_reverse(uint32_t c, uint32_t len) { return __brev(c) >> (32u - len); }

// LANE 0.  A[0, n): the counts of the used symbols, rising; S: their symbols.  -> len[symbol] <= max_bits for the used symbols (the
// others are left as they are: 0), num[l] = codes of length l.  Lengths of a minimum-redundancy code, derived in place (Moffat and
// Katajainen); lengths above max_bits are cut to it and the code is made complete again by lengthening, one at a time, a code of
// the largest length below max_bits that has one; lengths are then dealt out from the most frequent symbol down.
__device__ inline void gz_lengths(uint32_t *A, const uint16_t *S, int n, int max_bits, uint8_t *len, uint32_t *num)
{
	for (int l = 0; l < 16; ++l) num[l] = 0;
	if (n == 1) {
		len[S[0]] = 1;
		num[1] = 1;
		return;
	}
	A[0] += A[1];
	int root = 0, leaf = 2;
	for (int next = 1; next < n - 1; ++next) {
		if (leaf >= n || A[root] < A[leaf]) {
			A[next] = A[root];
			A[root++] = (uint32_t)next;
		} else
			A[next] = A[leaf++];
		if (leaf >= n || (root < next && A[root] < A[leaf])) {
			A[next] += A[root];
			A[root++] = (uint32_t)next;
		} else
			A[next] += A[leaf++];
	}
	A[n - 2] = 0;
	for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
	int avbl = 1, used = 0, dpth = 0, next = n - 1;
	root = n - 2;
	while (avbl > 0) {
		while (root >= 0 && (int)A[root] == dpth) {
			used++;
			root--;
		}
		while (avbl > used) {
			A[next--] = (uint32_t)dpth;
			avbl--;
		}
		avbl = 2 * used;
		dpth++;
		used = 0;
	}
	for (int i = 0; i < n; ++i) num[min((int)A[i], max_bits)]++;
	uint32_t total = 0;
	for (int l = 1; l <= max_bits; ++l) total += num[l] << (max_bits - l);
	while (total > (1u << max_bits)) {
		num[max_bits]--;
		for (int l = max_bits - 1; l > 0; --l)
			if (num[l]) {
				num[l]--;
				num[l + 1] += 2;
				break;
			}
		total--;
	}
	int j = n;
	for (int l = 1; l <= max_bits; ++l)
		for (uint32_t c = num[l]; c > 0; --c) len[S[--j]] = (uint8_t)l;
}

// LANE 0: canonical codes (RFC 1951, 3.2.2) from the lengths
__device__ inline void gz_codes(const uint8_t *len, int n_sym, int max_bits, const uint32_t *num, uint32_t *next, uint32_t *code)
{
	uint32_t c = 0;
	next[0] = 0;
	for (int l = 1; l <= max_bits; ++l) {
		c = (c + (l > 1 ? num[l - 1] : 0u)) << 1;
		next[l] = c;
	}
	for (int s = 0; s < n_sym; ++s) {
		const uint32_t l = len[s];
		code[s] = l ? (bit_reverse(next[l]++, l) | l << 16) : 0u;
	}
}

// all lanes: the used symbols of freq[0, n_sym) ranked by (count, symbol); *n_used has been zeroed behind a barrier
__device__ __forceinline__ void gz_rank(const uint32_t *freq, int n_sym, uint32_t *sortf, uint16_t *sorts, uint32_t *n_used)
{
	for (int s = (int)threadIdx.x; s < n_sym; s += kGzBlock) {
		const uint32_t f = freq[s];
		if (!f) continue;
		uint32_t r = 0;
		for (int q = 0; q < n_sym; ++q) {
			const uint32_t g = freq[q];
			r += (g != 0 && (g < f || (g == f && q < s))) ? 1u : 0u;
		}
		sortf[r] = f;
		sorts[r] = (uint16_t)s;
		atomicAdd(n_used, 1u);
	}
}

struct HeadWriter {
	uint32_t *w;
	uint32_t pos;
	__device__ __forceinline__ void put(uint32_t v, uint32_t n)
	{
		const uint32_t d = pos >> 5, sh = pos & 31u;
		w[d] |= v << sh;
		if (sh + n > 32u) w[d + 1] |= v >> (32u - sh);
		pos += n;
	}
};

// v (no bit at or above n, n <= 32) ORed in at bit `pos` of the zeroed slot
__device__ __forceinline__ void or_bits(uint32_t *slot, uint32_t pos, uint32_t v, uint32_t n)
{
	const uint32_t d = pos >> 5, sh = pos & 31u;
	if (v << sh) atomicOr(&slot[d], v << sh);
	if (sh + n > 32u && (v >> (32u - sh))) atomicOr(&slot[d + 1], v >> (32u - sh));
}

// LANE 0: the run-length coded sequence of the L.n_seq lengths of L.seq, the code of its symbols, the block header in L.head
__device__ inline void gz_block_header(GzLds &L)
{
	const int n_seq = (int)L.n_seq;
	// ---- runs: a run of zeros as 18s of up to 138 while 11 and more are left, then one 17 for 3..10, else single zeros; a run of
	// another length as the length itself, then 16s of up to 6 while 3 and more are left, then single lengths
	int n_tok = 0;
	for (int s = 0; s < kGzClSyms; ++s) L.cl_freq[s] = 0;
	for (int i = 0; i < n_seq;) {
		const uint32_t v = L.seq[i];
		int r = 1;
		while (i + r < n_seq && L.seq[i + r] == v) r++;
		i += r;
		if (v == 0) {
			while (r >= 11) {
				const int n = min(r, 138);
				L.cl_sym[n_tok] = 18, L.cl_extra[n_tok++] = (uint8_t)(n - 11);
				r -= n;
			}
			if (r >= 3) {
				L.cl_sym[n_tok] = 17, L.cl_extra[n_tok++] = (uint8_t)(r - 3);
				r = 0;
			}
		} else {
			L.cl_sym[n_tok] = (uint8_t)v, L.cl_extra[n_tok++] = 0;
			r--;
			while (r >= 3) {
				const int n = min(r, 6);
				L.cl_sym[n_tok] = 16, L.cl_extra[n_tok++] = (uint8_t)(n - 3);
				r -= n;
			}
		}
		for (; r > 0; --r) L.cl_sym[n_tok] = (uint8_t)v, L.cl_extra[n_tok++] = 0;
	}
	for (int t = 0; t < n_tok; ++t) L.cl_freq[L.cl_sym[t]]++;
	// ---- their code, 7 bits at the most; a lone symbol gets a partner of length 1 (symbol 0, or 1 if it is 0 itself)
	int n = 0;
	for (int s = 0; s < kGzClSyms; ++s) {
		L.cl_len[s] = 0;
		const uint32_t f = L.cl_freq[s];
		if (!f) continue;
		int at = n++;
		for (; at > 0 && L.cl_sortf[at - 1] > f; --at) L.cl_sortf[at] = L.cl_sortf[at - 1], L.cl_sorts[at] = L.cl_sorts[at - 1];
		L.cl_sortf[at] = f, L.cl_sorts[at] = (uint16_t)s;
	}
	gz_lengths(L.cl_sortf, L.cl_sorts, n, 7, L.cl_len, L.num);
	if (n == 1) {
		L.cl_len[L.cl_sorts[0] == 0 ? 1 : 0] = 1;
		L.num[1] = 2;
	}
	gz_codes(L.cl_len, kGzClSyms, 7, L.num, L.next, L.cl_code);
	int hclen = kGzClSyms;
	while (hclen > 4 && L.cl_len[kGzClOrder[hclen - 1]] == 0) hclen--;
	// ---- the header
	HeadWriter W{L.head, 0};
	W.put(1, 1);                    // BFINAL
	W.put(2, 2);                    // BTYPE: dynamic
	W.put(L.hlit - 257u, 5);        // HLIT
	W.put(L.hdist - 1u, 5);         // HDIST
	W.put((uint32_t)hclen - 4, 4);
	for (int i = 0; i < hclen; ++i) W.put(L.cl_len[kGzClOrder[i]], 3);
	for (int t = 0; t < n_tok; ++t) {
		const uint32_t s = L.cl_sym[t], c = L.cl_code[s];
		W.put(c & 0xFFFFu, c >> 16);
		if (s == 16) W.put(L.cl_extra[t], 2);
		if (s == 17) W.put(L.cl_extra[t], 3);
		if (s == 18) W.put(L.cl_extra[t], 7);
	}
	L.head_bits = W.pos;
}

// x8: x^(8 * 2^k) mod P for k < 16 (gzf::gz_powers).  sizes[m] for m < n_slots, 0 at m == n_slots (the scan runs over n_slots + 1
// entries).  n_slots = n_members + marker; slot n_members, if there is one, takes the end marker.
__global__ __launch_bounds__(kGzBlock) void k_gz_members(const uint4 *__restrict__ text, uint32_t n_bytes, uint32_t n_members, uint32_t n_slots,
                                                         uint32_t level, const uint32_t *__restrict__ x8, uint32_t *__restrict__ slots,
                                                         uint32_t *__restrict__ sizes, uint32_t *__restrict__ tokens,
                                                         unsigned long long *__restrict__ counters)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	GzLds &L = *reinterpret_cast<GzLds *>(lds_raw);
	const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid / kWave;
	L.crc_tab[tid] = 0;
	{
		uint32_t c = (uint32_t)tid;
		for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (gzf::kCrcPoly & (0u - (c & 1u)));
		L.crc_tab[tid] = c;
		if (tid < 16) L.x8[tid] = x8[tid];
	}
	if (blockIdx.x == 0 && tid == 0) sizes[n_slots] = 0;
#pragma unroll 1
	for (uint32_t m = blockIdx.x; m < n_slots; m += gridDim.x) {
		uint32_t *slot = slots + (size_t)m * (kGzSlot / 4);
		if (m == n_members) { // the end marker
			if (tid < (int)gzf::kGzMarker / 4) {
				const uint32_t w[7] = {0x04088b1fu, 0u, 0x0006ff00u, 0x00024342u, 0x0003001bu, 0u, 0u};
				uint32_t v = 0;
#pragma unroll
				for (int i = 0; i < 7; ++i) v = tid == i ? w[i] : v;
				slot[tid] = v;
			}
			if (tid == 0) sizes[m] = gzf::kGzMarker;
			continue;
		}
		const uint32_t base = m * kGzPiece, len = min(kGzPiece, n_bytes - base);
		__syncthreads(); // the round before has left LDS
		const long long t0 = clock64(); // (only lane 0's stamps are used)
		for (uint32_t v = (uint32_t)tid; v < (len + 15u) / 16u; v += kGzBlock) reinterpret_cast<uint4 *>(L.piece)[v] = text[base / 16u + v];
		for (int s = tid; s < kGzSymCap; s += kGzBlock) L.freq[s] = 0, L.len[s] = 0;
		if (tid < 32) L.dfreq[tid] = 0, L.dlen[tid] = 0;
		if (tid < kGzHeadWords) L.head[tid] = 0;
		if (tid == 0) L.n_used = 0, L.n_used_d = 0, L.head_bits = 0;
		if (level == 2) {
			for (int s = tid; s < (1 << kGzHashBits); s += kGzBlock) L.M.htab[s] = 0;
			if (tid == 0) L.M.entry = 0, L.M.n_tok = 0, L.M.n_match = 0, L.M.match_bytes = 0;
		}
		__syncthreads();
		// ---- a lane's slice: CRC state and histogram
		const uint32_t s0 = min(len, (uint32_t)tid * kGzLaneBytes), s1 = min(len, s0 + kGzLaneBytes);
		uint32_t crc = tid == 0 ? 0xFFFFFFFFu : 0u;
#pragma unroll 1
		for (uint32_t i = s0; i < s1; ++i) {
			const uint32_t b = L.piece[i];
			crc = L.crc_tab[(crc ^ b) & 0xFFu] ^ (crc >> 8);
			if (level == 1) atomicAdd(&L.freq[b], 1u);
		}
		{
			uint32_t p = 0x80000000u;
			const uint32_t tail = len - s1;
#pragma unroll 1
			for (int k = 0; k < 16; ++k)
				if ((tail >> k) & 1u) p = gzf::gz_mulmod(p, L.x8[k]);
			crc = gzf::gz_mulmod(crc, p);
		}
		for (int d = kWave / 2; d > 0; d >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, kWave);
		if (lane == 0) L.wave_crc[wave] = crc;
		if (tid == 0) L.freq[256] = 1; // end-of-block
		__syncthreads();
		crc = ~(L.wave_crc[0] ^ L.wave_crc[1] ^ L.wave_crc[2] ^ L.wave_crc[3]);
		long long t1 = clock64();
		const long long t_hist = t1 - t0;
		// ---- level 2: matches and the greedy parse, a chunk of the workgroup's width at a time
		uint32_t *tok = level == 2 ? tokens + (size_t)m * kGzPiece : nullptr; // a token per byte at the most
		if (level == 2) {
#pragma unroll 1
			for (uint32_t c0 = 0; c0 < len; c0 += kGzBlock) {
				const uint32_t i = c0 + (uint32_t)tid;
				const bool in = i < len, hashed = i + kGzMinMatch <= len;
				uint32_t h = 0, cand = 0;
				if (hashed) {
					h = ((L.piece[i] | (uint32_t)L.piece[i + 1] << 8 | (uint32_t)L.piece[i + 2] << 16) * 0x9E3779B1u) >> (32 - kGzHashBits);
					cand = L.M.htab[h]; // a position of an earlier chunk: this chunk inserts behind the barrier
				}
				const uint32_t entry = L.M.entry; // the first position no token covers yet
				__syncthreads();
				if (hashed) atomicMax(&L.M.htab[h], i + 1u);
				uint32_t ml = 0, md = 0;
				if (in && i >= entry) {
					const uint32_t maxl = min(kGzMaxMatch, len - i);
					if (maxl >= kGzMinMatch) {
						uint32_t la = 0, lb = 0;
						if (cand && i - (cand - 1u) <= kGzMaxDist) {
							const uint32_t j = cand - 1u;
							while (la < maxl && L.piece[j + la] == L.piece[i + la]) la++;
						}
						if (i >= 1u)
							while (lb < maxl && L.piece[i - 1u + lb] == L.piece[i + lb]) lb++;
						if (lb >= la && lb >= kGzMinMatch) ml = lb, md = 1u;
						else if (la > kGzMinMatch || (la == kGzMinMatch && i - (cand - 1u) <= kGzFar)) ml = la, md = i - (cand - 1u);
					}
				}
				const uint32_t step = ml ? ml : 1u;
				// the positions of the chunk on the path from `entry`: pointer jumping over jmp[t] = t + step
				L.M.jmp[tid] = (uint16_t)min((uint32_t)kGzBlock, (uint32_t)tid + step);
				L.M.sel[tid] = i == entry ? 1 : 0;
				__syncthreads();
#pragma unroll 1
				for (int k = 0; k < 8; ++k) {
					const uint32_t j = L.M.jmp[tid];
					if (L.M.sel[tid] && j < (uint32_t)kGzBlock) L.M.sel[j] = 1;
					const uint32_t j2 = j < (uint32_t)kGzBlock ? L.M.jmp[j] : (uint32_t)kGzBlock;
					__syncthreads();
					L.M.jmp[tid] = (uint16_t)j2;
					__syncthreads();
				}
				const bool chosen = in && L.M.sel[tid];
				const unsigned long long vote = __ballot(chosen);
				const uint32_t rank = (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
				if (lane == 0) L.M.wave_cnt[wave] = (uint32_t)__popcll(vote);
				if (chosen && (uint32_t)tid + step >= (uint32_t)kGzBlock) L.M.entry = i + step; // the last one on the path
				__syncthreads();
				uint32_t at = L.M.n_tok + rank, total = 0;
				for (int w = 0; w < kGzWaves; ++w) {
					if (w < wave) at += L.M.wave_cnt[w];
					total += L.M.wave_cnt[w];
				}
				if (chosen) {
					if (ml) {
						uint32_t ls, le, lx, ds, de, dx;
						len_symbol(ml, ls, le, lx);
						dist_symbol(md, ds, de, dx);
						tok[at] = 0x80000000u | (ml - 3u) << 15 | (md - 1u);
						atomicAdd(&L.freq[ls], 1u);
						atomicAdd(&L.dfreq[ds], 1u);
						atomicAdd(&L.M.n_match, 1u);
						atomicAdd(&L.M.match_bytes, ml);
					} else {
						tok[at] = L.piece[i];
						atomicAdd(&L.freq[L.piece[i]], 1u);
					}
				}
				__syncthreads(); // n_tok and wave_cnt have been read
				if (tid == 0) L.M.n_tok += total;
			}
			__syncthreads();
		}
		const long long t_match = level == 2 ? clock64() - t1 : 0;
		t1 += t_match;
		long long t2 = t1;
		// ---- codes
		uint32_t body_bits = 0, my_off = 0;
		if (level) {
			const int n_sym = level == 2 ? kGzLenSyms : kGzLitSyms;
			gz_rank(L.freq, n_sym, L.sortf, L.sorts, &L.n_used);
			gz_rank(L.dfreq, kGzDistSyms, L.dsortf, L.dsorts, &L.n_used_d);
			__syncthreads();
			if (tid == 0) {
				gz_lengths(L.sortf, L.sorts, (int)L.n_used, 15, L.len, L.num);
				gz_codes(L.len, n_sym, 15, L.num, L.next, L.code);
				// no distance symbol: one code of length 0; one: it gets length 1 (gz_lengths)
				if (L.n_used_d) {
					gz_lengths(L.dsortf, L.dsorts, (int)L.n_used_d, 15, L.dlen, L.num);
					gz_codes(L.dlen, kGzDistSyms, 15, L.num, L.next, L.dcode);
				}
				uint32_t hlit = 257, hdist = 1;
				for (int s = n_sym - 1; s >= 257; --s)
					if (L.len[s]) { hlit = (uint32_t)s + 1u; break; }
				for (int s = kGzDistSyms - 1; s >= 1; --s)
					if (L.dlen[s]) { hdist = (uint32_t)s + 1u; break; }
				for (uint32_t s = 0; s < hlit; ++s) L.seq[s] = L.len[s];
				for (uint32_t s = 0; s < hdist; ++s) L.seq[hlit + s] = L.dlen[s];
				L.hlit = hlit, L.hdist = hdist, L.n_seq = hlit + hdist;
				gz_block_header(L);
			}
			__syncthreads();
			t2 = clock64();
			uint32_t bits = 0;
			if (level == 2) { // a lane's slice of the tokens
				const uint32_t per = (L.M.n_tok + kGzBlock - 1u) / kGzBlock, a = min(L.M.n_tok, (uint32_t)tid * per), b = min(L.M.n_tok, a + per);
#pragma unroll 1
				for (uint32_t k = a; k < b; ++k) bits += token_bits(L, tok[k]);
			} else {
#pragma unroll 1
				for (uint32_t i = s0; i < s1; ++i) bits += L.code[L.piece[i]] >> 16;
			}
			uint32_t incl = bits;
			for (int d = 1; d < kWave; d <<= 1) {
				const uint32_t o = __shfl_up(incl, d, kWave);
				if (lane >= d) incl += o;
			}
			if (lane == kWave - 1) L.wave_bits[wave] = incl;
			__syncthreads();
			my_off = incl - bits;
			for (int w = 0; w < kGzWaves; ++w) {
				if (w < wave) my_off += L.wave_bits[w];
				body_bits += L.wave_bits[w];
			}
		}
		const uint32_t eob = level ? L.code[256] : 0u, total_bits = L.head_bits + body_bits + (eob >> 16);
		const uint32_t dyn_bytes = (total_bits + 7u) / 8u, stored_bytes = gzf::kGzStoredHead + len;
		const bool dyn = level != 0 && dyn_bytes < stored_bytes;
		const uint32_t size = gzf::kGzHead + (dyn ? dyn_bytes : stored_bytes) + gzf::kGzTail;
		const uint32_t tail_at = size - gzf::kGzTail; // byte the trailer starts at
		if (dyn) {
			for (uint32_t w = (uint32_t)tid; w < (size + 3u) / 4u; w += kGzBlock) slot[w] = 0;
			__syncthreads(); // the zeros are in place before any lane of the workgroup ORs into them
			// a lane's slice: bits gather in `acc` from bit `have` of dword `d` on
			const uint32_t start = gzf::kGzHead * 8u + L.head_bits + my_off;
			uint32_t d = start >> 5, have = start & 31u;
			unsigned long long acc = 0;
			bool first = true;
			auto put = [&](uint32_t v, uint32_t n) { // n <= 32 bits behind the `have` < 32 that wait
				acc |= (unsigned long long)v << have;
				have += n;
				if (have >= 32u) {
					const uint32_t out = (uint32_t)acc;
					if (first) {
						if (out) atomicOr(&slot[d], out);
					} else
						slot[d] = out;
					first = false;
					d++;
					acc >>= 32;
					have -= 32u;
				}
			};
			if (level == 2) {
				const uint32_t per = (L.M.n_tok + kGzBlock - 1u) / kGzBlock, a = min(L.M.n_tok, (uint32_t)tid * per), b = min(L.M.n_tok, a + per);
#pragma unroll 1
				for (uint32_t k = a; k < b; ++k) {
					const uint32_t t = tok[k];
					if (!(t >> 31)) {
						put(L.code[t] & 0xFFFFu, L.code[t] >> 16);
						continue;
					}
					uint32_t ls, le, lx, ds, de, dx;
					len_symbol(((t >> 15) & 0xFFu) + 3u, ls, le, lx);
					dist_symbol((t & 0x7FFFu) + 1u, ds, de, dx);
					const uint32_t lc = L.code[ls], dc = L.dcode[ds];
					put((lc & 0xFFFFu) | lx << (lc >> 16), (lc >> 16) + le);
					put((dc & 0xFFFFu) | dx << (dc >> 16), (dc >> 16) + de);
				}
			} else {
#pragma unroll 1
				for (uint32_t i = s0; i < s1; ++i) {
					const uint32_t c = L.code[L.piece[i]];
					put(c & 0xFFFFu, c >> 16);
				}
			}
			if ((uint32_t)acc) atomicOr(&slot[d], (uint32_t)acc);
			// header, block header, end-of-block, trailer
			if (tid < 4) or_bits(slot, 32u * tid, tid == 0 ? 0x04088b1fu : tid == 1 ? 0u : tid == 2 ? 0x0006ff00u : 0x00024342u, 32);
			if (tid == 4) or_bits(slot, 128, size - 1u, 16);
			for (uint32_t w = (uint32_t)tid; w < (L.head_bits + 31u) / 32u; w += kGzBlock) or_bits(slot, gzf::kGzHead * 8u + 32u * w, L.head[w], 32);
			if (tid == 5) or_bits(slot, gzf::kGzHead * 8u + L.head_bits + body_bits, eob & 0xFFFFu, eob >> 16);
			if (tid == 6) or_bits(slot, tail_at * 8u, crc, 32);
			if (tid == 7) or_bits(slot, tail_at * 8u + 32u, len, 32);
		} else {
			// stored: 01 | LEN | ~LEN | the piece; a thread composes one dword of the slot at a time
			for (uint32_t w = (uint32_t)tid; w < (size + 3u) / 4u; w += kGzBlock) {
				uint32_t v = 0;
#pragma unroll
				for (uint32_t j = 0; j < 4; ++j) {
					const uint32_t at = 4u * w + j;
					uint32_t b = 0;
					if (at < 16u) b = (at == 0 ? 0x1fu : at == 1 ? 0x8bu : at == 2 ? 0x08u : at == 3 ? 0x04u : at == 9 ? 0xffu : at == 10 ? 0x06u : at == 12 ? 0x42u : at == 13 ? 0x43u : at == 14 ? 0x02u : 0u);
					else if (at < 18u) b = ((size - 1u) >> (8u * (at - 16u))) & 0xFFu;
					else if (at == 18u) b = 1u;
					else if (at < 21u) b = (len >> (8u * (at - 19u))) & 0xFFu;
					else if (at < 23u) b = ((~len) >> (8u * (at - 21u))) & 0xFFu;
					else if (at < tail_at) b = L.piece[at - 23u];
					else if (at < tail_at + 4u) b = (crc >> (8u * (at - tail_at))) & 0xFFu;
					else if (at < size) b = (len >> (8u * (at - tail_at - 4u))) & 0xFFu;
					v |= b << (8u * j);
				}
				slot[w] = v;
			}
		}
		if (tid == 0) {
			sizes[m] = size;
			if (!dyn) atomicAdd(&counters[GC_STORED], 1ull);
			else if (level == 2) {
				atomicAdd(&counters[GC_LITERALS], (unsigned long long)(L.M.n_tok - L.M.n_match));
				atomicAdd(&counters[GC_MATCHES], (unsigned long long)L.M.n_match);
				atomicAdd(&counters[GC_MATCH_BYTES], (unsigned long long)L.M.match_bytes);
			} else
				atomicAdd(&counters[GC_LITERALS], (unsigned long long)len);
			atomicAdd(&counters[GC_CYC_HIST], (unsigned long long)t_hist);
			atomicAdd(&counters[GC_CYC_MATCH], (unsigned long long)t_match);
			atomicAdd(&counters[GC_CYC_CODES], (unsigned long long)(t2 - t1));
			atomicAdd(&counters[GC_CYC_ENCODE], (unsigned long long)(clock64() - t2));
		}
	}
}

// off: the exclusive scan of the sizes, n_slots + 1 entries.  A workgroup copies a member: no byte of out outside it is written.
__global__ __launch_bounds__(kGzBlock) void k_gz_gather(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ off, uint32_t n_slots,
                                                        uint8_t *__restrict__ out)
{
	const uint32_t tid = threadIdx.x;
#pragma unroll 1
	for (uint32_t m = blockIdx.x; m < n_slots; m += gridDim.x) {
		const uint64_t o = off[m];
		const uint32_t size = (uint32_t)(off[m + 1] - o);
		const uint8_t *src = slots + (size_t)m * kGzSlot;
		const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
		// up to 3 bytes in front of the first dword boundary of the output, whole dwords, up to 3 bytes behind them
		const uint32_t head = min(size, (uint32_t)((4u - (o & 3u)) & 3u)), words = (size - head) / 4u, tail_at = head + 4u * words;
		if (tid < head) out[o + tid] = src[tid];
		uint32_t *dst = reinterpret_cast<uint32_t *>(out + o + head);
		const uint32_t sh = 8u * head;
		for (uint32_t w = tid; w < words; w += kGzBlock) dst[w] = sh ? (src32[w] >> sh) | (src32[w + 1] << (32u - sh)) : src32[w];
		if (tid < size - tail_at) out[o + tail_at + tid] = src[tail_at + tid];
	}
}

} // namespace gzk
} // namespace dbgk
