// INFLATE stage (include/dbgk.h, INFLATE section; the decode core in dbgk_inflate_core.h; framing in dbgk_gz_frame.h; host side
// dbgk_host_inflate.h): BGZF-framed gzip members become their bytes, members back to back.  The caller's table says
// where every member starts.  The bit-serial part and the parallel part are two kernels, with the deflater's tokens between them.
//
//   k_inf_sizes    a lane per member: the frame check, ISIZE and CRC-32 out of the trailer, end markers counted
//   (scan)         ISIZE -> the members' places in the output (dbgk_sort.hip, rocPRIM)
//   k_inf_decode   a workgroup is ONE wave that holds kInfLanes members, one decoding lane each: bits -> table lookup -> consume is
//                  serial within a member, so the parallelism is members.  A decoder's tables (inf::InfTables, 2 080 bytes) lie in
//                  LDS; it reads its member's stream byte by byte through the core's checked bit reader and writes 4-byte tokens to
//                  the member's slot of the token area, never more than ISIZE of them.
//   k_inf_resolve  ONE workgroup per member turns tokens into bytes in an LDS image of the member's output: 256 tokens at a time,
//                  a scan of their lengths gives the positions, literals are placed by all lanes at once, the matches of the chunk
//                  are copied in token order with the lanes parallel inside a match (src = p - dist + i mod dist covers overlap);
//                  then the CRC-32 as the deflater computes it (a slice per lane by table, brought to the end by x^(8 tail) mod P,
//                  XORed over the workgroup) against the trailer's; then the image leaves in 16-byte vectors.  A member with a
//                  verdict other than 0 leaves as zeros.
//
// Rounds: the token area holds kInfRound members (kInfTokenBytes, below 1 GiB, whatever the call's size); the host launches decode and
// resolve once per round.  No kernel waits for another workgroup, and a workgroup handles one member (resolve) or one group of
// members (decode) and ends: nothing is carried from one member to another.
// Memory: a member's bytes are read inside [offset, offset + size) only, its tokens written inside its slot, its output inside
// [place, place + ISIZE): each is checked before the access, by the core for the decode and here for the rest.
#pragma once

#ifndef DBGK_GZ_HD
#define DBGK_GZ_HD __host__ __device__
#endif
#include "dbgk_inflate_core.h"
#include "dbgk_emit.h"

namespace dbgk {
namespace infk {

using emitk::kWave;
using emitk::lane_id;
using gzf::kGzPiece;

constexpr int kInfLanes = 16;                 // decoders per workgroup of one wave: 33 280 bytes of LDS, four workgroups per CU
constexpr int kInfDecodeBlock = kWave;
constexpr int kInfBlock = 256;                // k_inf_resolve, k_inf_sizes
constexpr int kInfWaves = kInfBlock / kWave;
constexpr uint32_t kInfRound = 4000;          // members per round
constexpr uint64_t kInfTokenBytes = (uint64_t)kInfRound * kGzPiece * 4u; // 1 044 480 000: the stage's temporary memory
static_assert(kInfTokenBytes <= (1ull << 30), "the token area stays below 1 GiB");
constexpr uint32_t kInfLaneBytes = kGzPiece / kInfBlock; // 255: a lane's slice of the CRC

enum Counter { IC_MARKERS = 0, IC_STORED, IC_FIXED, IC_DYNAMIC, IC_LITERALS, IC_MATCHES, IC_COUNT };

struct InfResolveLds {
	uint8_t img[kGzPiece + 16];  // (the 16: an unaligned dword read of the last bytes stays inside)
	uint32_t crc_tab[256];
	uint32_t x8[16];
	uint32_t mpos[kInfBlock];    // the matches of a chunk, in token order: position, and length << 16 | distance - 1
	uint32_t mtok[kInfBlock];
	uint32_t wave_len[kInfWaves], wave_cnt[kInfWaves], wave_crc[kInfWaves];
	uint32_t bad;
};

// off: n_members + 1 offsets into gz, non-decreasing, the last one inside the buffer (the host has checked).  -> isize[m] (0 for a
// member that is not the framing, and at m == n_members), crc[m], status[m] = 0 or R_FRAME
__global__ __launch_bounds__(kInfBlock) void k_inf_sizes(const uint8_t *__restrict__ gz, const uint64_t *__restrict__ off, uint32_t n_members,
                                                        uint32_t *__restrict__ isize, uint32_t *__restrict__ crc, uint32_t *__restrict__ status,
                                                        unsigned long long *__restrict__ counters)
{
	const uint32_t m = blockIdx.x * kInfBlock + threadIdx.x;
	if (m == n_members) isize[m] = 0;
	if (m >= n_members) return;
	const uint64_t o = off[m], size = off[m + 1] - o;
	uint32_t n = 0, c = 0;
	const uint32_t r = inf::inf_frame(gz + o, size, &n, &c); // reads nothing unless 28 <= size <= 65 536
	isize[m] = n;
	crc[m] = c;
	status[m] = r;
	if (!r && size == gzf::kGzMarker && n == 0 && c == 0 && gz[o + 18] == 3 && gz[o + 19] == 0) atomicAdd(&counters[IC_MARKERS], 1ull);
}

// members [r0, r0 + nr) of the call: member r0 + j decodes into slot j of the token area
__global__ __launch_bounds__(kInfDecodeBlock) void k_inf_decode(const uint8_t *__restrict__ gz, const uint64_t *__restrict__ off, const uint32_t *__restrict__ isize,
                                                               uint32_t r0, uint32_t nr, uint32_t *__restrict__ tokens, uint32_t *__restrict__ n_tok,
                                                               uint32_t *__restrict__ status, unsigned long long *__restrict__ counters)
{
	__shared__ inf::InfTables T[kInfLanes];
	const uint32_t lane = threadIdx.x, j = blockIdx.x * kInfLanes + lane;
	if (lane >= (uint32_t)kInfLanes || j >= nr) return;
	const uint32_t m = r0 + j;
	n_tok[j] = 0;
	if (status[m]) return;
	const uint64_t o = off[m];
	const uint32_t size = (uint32_t)(off[m + 1] - o); // 28..65 536: the frame check has passed
	inf::InfCount C{};
	uint32_t nt = 0;
	const uint32_t r = inf::inf_decode(gz + o + gzf::kGzHead, size - gzf::kGzHead - gzf::kGzTail, isize[m], tokens + (size_t)j * kGzPiece, T[lane], &nt, C);
	n_tok[j] = nt;
	status[m] = r;
	if (r) return;
	if (C.n_stored) atomicAdd(&counters[IC_STORED], (unsigned long long)C.n_stored);
	if (C.n_fixed) atomicAdd(&counters[IC_FIXED], (unsigned long long)C.n_fixed);
	if (C.n_dynamic) atomicAdd(&counters[IC_DYNAMIC], (unsigned long long)C.n_dynamic);
	if (C.n_literals) atomicAdd(&counters[IC_LITERALS], (unsigned long long)C.n_literals);
	if (C.n_matches) atomicAdd(&counters[IC_MATCHES], (unsigned long long)C.n_matches);
}

// an unaligned dword of the image
__device__ __forceinline__ uint32_t img_dword(const uint8_t *img, uint32_t at)
{
	const uint32_t *I = reinterpret_cast<const uint32_t *>(img);
	const uint32_t w = at >> 2, s = (at & 3u) * 8u, lo = I[w];
	return s ? (lo >> s) | (I[w + 1] << (32u - s)) : lo;
}

// place: the exclusive scan of isize, n_members + 1 entries.  Writes out[place[m], place[m] + isize[m]) and nothing else of out.
__global__ __launch_bounds__(kInfBlock) void k_inf_resolve(const uint32_t *__restrict__ tokens, const uint32_t *__restrict__ n_tok,
                                                          const uint32_t *__restrict__ isize, const uint32_t *__restrict__ crc,
                                                          const uint64_t *__restrict__ place, const uint32_t *__restrict__ x8, uint32_t r0,
                                                          uint32_t *__restrict__ status, uint8_t *__restrict__ out)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	InfResolveLds &L = *reinterpret_cast<InfResolveLds *>(lds_raw);
	const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wave = tid / kWave, j = blockIdx.x, m = r0 + j;
	const uint32_t len = min(isize[m], kGzPiece), n = min(n_tok[j], len); // (a token stands for a byte at least)
	const uint32_t *tok = tokens + (size_t)j * kGzPiece;
	bool good = status[m] == 0;
	{
		uint32_t c = tid;
		for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (gzf::kCrcPoly & (0u - (c & 1u)));
		L.crc_tab[tid] = c;
		if (tid < 16) L.x8[tid] = x8[tid];
		if (tid == 0) L.bad = 0;
	}
	__syncthreads();
	if (good) {
		uint32_t base = 0;
#pragma unroll 1
		for (uint32_t c0 = 0; c0 < n; c0 += kInfBlock) {
			const bool in = c0 + tid < n;
			const uint32_t t = in ? tok[c0 + tid] : 0u;
			const bool match = in && (t >> 31);
			const uint32_t tl = !in ? 0u : match ? ((t >> 15) & 0xFFu) + 3u : 1u;
			uint32_t incl = tl;
			for (int d = 1; d < kWave; d <<= 1) {
				const uint32_t o = __shfl_up(incl, d, kWave);
				if (lane >= (uint32_t)d) incl += o;
			}
			const unsigned long long vote = __ballot(match);
			if (lane == (uint32_t)kWave - 1u) L.wave_len[wave] = incl;
			if (lane == 0) L.wave_cnt[wave] = (uint32_t)__popcll(vote);
			__syncthreads();
			uint32_t pos = base + incl - tl, rank = (uint32_t)__popcll(vote & ((1ull << lane) - 1ull)), total = 0, n_match = 0;
			for (uint32_t w = 0; w < (uint32_t)kInfWaves; ++w) {
				if (w < wave) pos += L.wave_len[w], rank += L.wave_cnt[w];
				total += L.wave_len[w];
				n_match += L.wave_cnt[w];
			}
			if (in) {
				const uint32_t dist = (t & 0x7FFFu) + 1u;
				const bool ok = pos + tl <= len && (!match || dist <= pos); // (the decoder refuses a member with another token)
				if (!ok) L.bad = 1;
				if (match) L.mpos[rank] = ok ? pos : 0u, L.mtok[rank] = ok ? tl << 16 | (dist - 1u) : 0u; // else: a match of no bytes
				else if (ok) L.img[pos] = (uint8_t)t;
			}
			__syncthreads();
#pragma unroll 1
			for (uint32_t k = 0; k < n_match; ++k) {
				const uint32_t p = L.mpos[k], ml = L.mtok[k] >> 16, dist = (L.mtok[k] & 0xFFFFu) + 1u;
				for (uint32_t i = tid; i < ml; i += kInfBlock) L.img[p + i] = L.img[p - dist + i % dist];
				__syncthreads();
			}
			base += total;
		}
		__syncthreads();
		if (L.bad || base != len) good = false; // (base: uniform)
		// ---- CRC-32: a lane's slice, brought to the end of the member
		const uint32_t s0 = min(len, tid * kInfLaneBytes), s1 = min(len, s0 + kInfLaneBytes);
		uint32_t c = tid == 0 ? 0xFFFFFFFFu : 0u;
#pragma unroll 1
		for (uint32_t i = s0; i < s1; ++i) c = L.crc_tab[(c ^ L.img[i]) & 0xFFu] ^ (c >> 8);
		{
			uint32_t p = 0x80000000u;
			const uint32_t tail = len - s1;
#pragma unroll 1
			for (int k = 0; k < 16; ++k)
				if ((tail >> k) & 1u) p = gzf::gz_mulmod(p, L.x8[k]);
			c = gzf::gz_mulmod(c, p);
		}
		for (int d = kWave / 2; d > 0; d >>= 1) c ^= (uint32_t)__shfl_xor((int)c, d, kWave);
		if (lane == 0) L.wave_crc[wave] = c;
		__syncthreads();
		c = ~(L.wave_crc[0] ^ L.wave_crc[1] ^ L.wave_crc[2] ^ L.wave_crc[3]);
		if (good && c != crc[m]) {
			good = false;
			if (tid == 0) status[m] = inf::R_CRC;
		} else if (!good && tid == 0)
			status[m] = inf::R_OUT_MORE;
	}
	if (!good) { // a refused member leaves as zeros
		__syncthreads();
		for (uint32_t w = tid; w < (len + 19u) / 4u; w += kInfBlock) reinterpret_cast<uint32_t *>(L.img)[w] = 0;
		__syncthreads();
	}
	// ---- the image to its place: up to 15 bytes in front of the first 16-byte boundary of the output, whole vectors, the rest
	const uint64_t o = place[m];
	const uint32_t head = min(len, (uint32_t)((16u - (o & 15u)) & 15u)), vecs = (len - head) / 16u, tail_at = head + 16u * vecs;
	if (tid < head) out[o + tid] = L.img[tid];
	uint4 *dst = reinterpret_cast<uint4 *>(out + o + head);
	for (uint32_t v = tid; v < vecs; v += kInfBlock) {
		const uint32_t at = head + 16u * v;
		dst[v] = make_uint4(img_dword(L.img, at), img_dword(L.img, at + 4u), img_dword(L.img, at + 8u), img_dword(L.img, at + 12u));
	}
	if (tid < len - tail_at) out[o + tail_at + tid] = L.img[tail_at + tid];
}

} // namespace infk
} // namespace dbgk
