// dbgk_map.h -- MAP: map_reads / map_pair of the link_scaffold module on the GPU (gfx950 only).
//
// Reference semantics (files of the reference's link_scaffold/ directory):
//   get_align_seed        map_func.cpp:181-237   two unique k-mers SeedKmerNum apart locate and orient the read
//   extend_align_region   map_func.cpp:241-299   gap-free extension to the read's or the contig's end, mismatches counted
//   seq2bit               seqKmer.cpp:36-43      codes are OR-ed in UNMASKED: a byte outside ACGTacgtNn has code 4
//   rev_com_seq           seqKmer.cpp:83-91      c -> c_bases[alphabet[c]], N / n kept
//   second alignment      map_reads.cpp:480-498
//
// One read per wave, four reads per workgroup.  The read is staged in LDS (reads of up to kMapSlice bytes; longer ones
// are listed and mapped by the same code out of global memory).  The index is the finalized SEEDIDX table in its
// build-time payload form (dbgk_kernels.h: id << 32 | (pos + 1) << 2 | direct << 1 | dup, key 0 beside the table).
#pragma once

#include "dbgk_kernels.h"

namespace dbgk {
namespace mapk {

constexpr int kMapWaves = 4;          // reads per workgroup
constexpr uint32_t kMapSlice = 1024;  // longest read that is mapped out of LDS
constexpr uint32_t kMapSliceBytes = kMapSlice + 16; // the slice starts at the dword below the read's first byte

struct MapParams {
	int32_t k, s, min_read_len, second;
	uint32_t chunk0;            // windows probed together at the start of a scan; 64 from then on
	uint32_t n_accept;          // entries of `accept`
};

struct MapIndex {
	TableRef T;
	uint64_t key0;              // payload of key 0 (0 = absent), which lives beside the table
	const uint8_t *ctg;         // contig text, ASCII as written
	const uint64_t *ctg_off;    // [n_contigs + 1]
	uint32_t n_contigs;
};

// device counters of one batch
struct MapCounters {
	unsigned long long by_lds, by_long, skipped, windows;
	unsigned int n_long, pad;
};

struct Hit { // == dbgk_map_hit
	int32_t contig, read_start, read_end, contig_start, contig_end, mismatches, align_len, direct;
};

// alphabet[] of seqKmer.cpp:11-21 for bytes below 128; bytes from 128 on (an out-of-bounds read there) count as 4 too
__device__ __forceinline__ uint32_t map_code(uint32_t c)
{
	const uint32_t u = c & 0xDFu;
	const bool letter = c < 128u && (u == 0x41u || u == 0x43u || u == 0x47u || u == 0x54u || u == 0x4Eu);
	return letter ? ((c >> 1) ^ (c >> 2)) & 3u : 4u;
}

// one byte of rev_com_seq (seqKmer.cpp:83-91)
__device__ __forceinline__ uint32_t map_complement(uint32_t c)
{
	if (c == 'N' || c == 'n') return c;
	const uint32_t code = map_code(c);
	return (uint32_t)(0x4E41434754ull >> (8u * code)) & 0xFFu; // "TGCAN"[code]
}

// the read of a wave: bytes out of LDS or out of global memory
struct LdsRead {
	const uint8_t *p;
	__device__ __forceinline__ uint32_t at(uint32_t i) const { return p[i]; }
};
struct GlobalRead {
	const uint8_t *p;
	__device__ __forceinline__ uint32_t at(uint32_t i) const { return p[i]; }
};

// seq2bit of the window at i, its reverse complement, the canonical pick (map_func.cpp:188-199)
template <class R>
__device__ __forceinline__ uint64_t map_window_key(const R &rd, uint32_t i, int k, uint32_t &direct)
{
	uint64_t kbit = 0;
	for (int j = 0; j < k; j++) kbit = (kbit << 2) | map_code(rd.at(i + (uint32_t)j));
	const uint64_t rc = revcomp_kbit(kbit, k);
	direct = kbit < rc ? 1u : 0u;
	return direct ? kbit : rc;
}

// exist_kmerset (kmerSet.cpp:216-238): payload of the key, 0 when absent
__device__ __forceinline__ uint64_t map_lookup(const MapIndex &X, uint64_t key)
{
	if (key == 0ull) return X.key0;
	uint64_t slot = fast_mod(hash_code(key), X.T.magic);
	for (uint64_t steps = 0; steps < X.T.size; steps++) {
		const uint4 v = *reinterpret_cast<const uint4 *>(&X.T.nodes[slot]);
		const uint64_t kmer = ((uint64_t)v.y << 32) | v.x;
		if (kmer == key) return ((uint64_t)v.w << 32) | v.z;
		if (kmer == 0ull) return 0ull;
		slot = (slot + 1 == X.T.size) ? 0 : slot + 1;
	}
	return 0ull;
}

// get_align_seed over the windows first .. last (0-based starts): true when a seed was found, `h` then holds it
template <class R>
__device__ bool map_seed_scan(const R &rd, const MapParams &P, const MapIndex &X, int32_t first, int32_t last, Hit &h,
                              unsigned long long &windows)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t chunk = P.chunk0;
	for (int64_t base = first; base <= (int64_t)last; base += chunk, chunk = 64u) {
		const int64_t i = base + lane;
		const bool active = lane < chunk && i <= (int64_t)last;
		bool found = false;
		uint64_t w1 = 0, w2 = 0;
		uint32_t d1 = 0;
		if (active) {
			const uint64_t key = map_window_key(rd, (uint32_t)i, P.k, d1);
			w1 = map_lookup(X, key);
			if (w1 != 0ull && (w1 & 1ull) == 0ull) { // present and freq == 1
				uint32_t d2;
				const uint64_t key2 = map_window_key(rd, (uint32_t)i + (uint32_t)P.s, P.k, d2);
				w2 = map_lookup(X, key2);
				if (w2 != 0ull && (w2 & 1ull) == 0ull && (w2 >> 32) == (w1 >> 32)) {
					const int64_t p1 = (int64_t)((w1 >> 2) & 0x3FFFFFFFull), p2 = (int64_t)((w2 >> 2) & 0x3FFFFFFFull);
					const int64_t d = p2 > p1 ? p2 - p1 : p1 - p2;
					found = d == (int64_t)P.s;
				}
			}
		}
		const unsigned long long act = __ballot(active), hits = __ballot(found);
		if (hits) {
			const int src = __ffsll((long long)hits) - 1; // the reference's first i (break at :232)
			windows += (unsigned long long)__popcll(act);
			const uint64_t a = __shfl(w1, src, 64), b = __shfl(w2, src, 64);
			const uint32_t dr = __shfl(d1, src, 64);
			const int32_t pos = (int32_t)((a >> 2) & 0x3FFFFFFFull) - 1, pos2 = (int32_t)((b >> 2) & 0x3FFFFFFFull) - 1;
			const int32_t at = (int32_t)(base + src);
			const bool fwd = dr == (uint32_t)((a >> 1) & 1ull);
			h.contig = (int32_t)(a >> 32);
			h.contig_start = fwd ? pos + 1 : pos2 + 1;
			h.contig_end = fwd ? pos2 + P.k : pos + P.k;
			h.direct = fwd ? 'F' : 'R';
			h.read_start = at + 1;
			h.read_end = at + P.s + P.k;
			return true;
		}
		windows += (unsigned long long)__popcll(act);
	}
	return false;
}

// extend_align_region + the identity test; h.contig becomes -1 when the alignment is rejected
template <class R>
__device__ void map_extend(const R &rd, int32_t L, const MapParams &P, const MapIndex &X, const int32_t *__restrict__ accept, Hit &h)
{
	const uint32_t lane = threadIdx.x & 63u;
	const bool rev = h.direct == 'R';
	int32_t rs = h.read_start, re = h.read_end, cs = h.contig_start, ce = h.contig_end;
	int32_t align_len = re - rs + 1, mis = 0;
	if (rev) {
		const int32_t a = L - rs + 1, b = L - re + 1;
		rs = b;
		re = a;
	}
	const bool known = (uint32_t)h.contig < X.n_contigs;
	const uint64_t c0 = known ? X.ctg_off[h.contig] : 0ull;
	const int64_t C = known ? (int64_t)(X.ctg_off[h.contig + 1] - c0) : 0;
	const uint8_t *ctg = X.ctg + c0;
	auto read_at = [&](int32_t p) -> uint32_t { // byte p (0-based) of the read as the extension sees it
		return rev ? map_complement(rd.at((uint32_t)(L - 1 - p))) : rd.at((uint32_t)p);
	};
	// leftward: read[rs - 1 - t] against contig[cs - 1 - t], t = 1 .. nl
	int64_t nl = (int64_t)rs - 1 < (int64_t)cs - 1 ? (int64_t)rs - 1 : (int64_t)cs - 1;
	if (nl < 0 || (int64_t)cs - 1 > C) nl = 0;
	for (int64_t t0 = 1; t0 <= nl; t0 += 64) {
		const int64_t t = t0 + lane;
		const bool bad = t <= nl && read_at((int32_t)(rs - 1 - t)) != (uint32_t)ctg[cs - 1 - t];
		mis += __popcll(__ballot(bad));
	}
	rs -= (int32_t)nl;
	cs -= (int32_t)nl;
	// rightward: read[re - 1 + t] against contig[ce - 1 + t], t = 1 .. nr
	int64_t nr = (int64_t)L - re < C - (int64_t)ce ? (int64_t)L - re : C - (int64_t)ce;
	if (nr < 0 || ce < 1) nr = 0;
	for (int64_t t0 = 1; t0 <= nr; t0 += 64) {
		const int64_t t = t0 + lane;
		const bool bad = t <= nr && read_at((int32_t)(re - 1 + t)) != (uint32_t)ctg[ce - 1 + t];
		mis += __popcll(__ballot(bad));
	}
	re += (int32_t)nr;
	ce += (int32_t)nr;
	align_len += (int32_t)(nl + nr);
	if (rev) {
		const int32_t a = L - rs + 1, b = L - re + 1;
		rs = b;
		re = a;
	}
	h.read_start = rs;
	h.read_end = re;
	h.contig_start = cs;
	h.contig_end = ce;
	h.mismatches = mis;
	h.align_len = align_len;
	// identity: the host's table holds, per align_len, the largest mismatch count the reference's float test accepts
	const int32_t most = (align_len >= 0 && (uint32_t)align_len < P.n_accept) ? accept[align_len] : -1;
	if (mis > most) h.contig = -1;
}

__device__ __forceinline__ Hit map_no_hit()
{
	return Hit{-1, -1, -1, -1, -1, 0, 0, 'N'};
}

template <class R>
__device__ void map_one(const R &rd, int32_t L, const MapParams &P, const MapIndex &X, const int32_t *__restrict__ accept, Hit *__restrict__ out,
                        unsigned long long &windows)
{
	Hit h1 = map_no_hit(), h2 = map_no_hit();
	if (L >= P.min_read_len && L >= P.k + P.s) {
		if (map_seed_scan(rd, P, X, 0, L - P.k - P.s, h1, windows)) map_extend(rd, L, P, X, accept, h1);
		if (P.second && h1.contig != -1 && h1.read_end < L && L - h1.read_end >= P.k + P.s) {
			if (map_seed_scan(rd, P, X, h1.read_end, L - P.k - P.s, h2, windows)) map_extend(rd, L, P, X, accept, h2);
		}
	}
	if ((threadIdx.x & 63u) == 0u) {
		out[0] = h1;
		out[1] = h2;
	}
}

// LONG = false: every read of the batch, one per wave; reads longer than kMapSlice are appended to long_list.
// LONG = true : the listed reads out of global memory.
template <bool LONG>
__global__ __launch_bounds__(kMapWaves * 64) void k_map_reads(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ off, uint32_t n_reads,
                                                                MapParams P, MapIndex X, const int32_t *__restrict__ accept,
                                                                Hit *__restrict__ hits, uint32_t *__restrict__ long_list,
                                                                MapCounters *__restrict__ ctr)
{
	__shared__ __attribute__((aligned(16))) uint8_t lds[LONG ? 16 : kMapWaves * kMapSliceBytes];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t n_items = LONG ? ctr->n_long : n_reads;
	unsigned long long windows = 0, done = 0, skipped = 0;
	for (uint64_t item = (uint64_t)blockIdx.x * kMapWaves + wave; item < n_items; item += (uint64_t)gridDim.x * kMapWaves) {
		const uint32_t r = LONG ? long_list[item] : (uint32_t)item;
		const uint64_t o = off[r];
		const uint64_t len64 = off[r + 1] - o;
		const int32_t L = (int32_t)len64; // < 2^31, checked by the host
		if (L < P.min_read_len || L < P.k + P.s) { // two empty hits
			if (lane == 0) {
				hits[2 * (uint64_t)r] = map_no_hit();
				hits[2 * (uint64_t)r + 1] = map_no_hit();
			}
			skipped++;
			continue;
		}
		if (LONG) {
			map_one(GlobalRead{seq + o}, L, P, X, accept, hits + 2 * (uint64_t)r, windows);
			done++;
		} else {
			if (len64 > kMapSlice) {
				if (lane == 0) long_list[atomicAdd(&ctr->n_long, 1u)] = r;
				continue;
			}
			uint8_t *slice = lds + wave * kMapSliceBytes;
			const uint64_t a0 = o & ~3ull; // whole dwords from the one that holds the first byte (the batch buffer has 16 spare bytes)
			const uint32_t shift = (uint32_t)(o - a0), n_dw = (shift + (uint32_t)L + 3u) >> 2;
			for (uint32_t w = lane; w < n_dw; w += 64u)
				reinterpret_cast<uint32_t *>(slice)[w] = *reinterpret_cast<const uint32_t *>(seq + a0 + 4ull * w);
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			map_one(LdsRead{slice + shift}, L, P, X, accept, hits + 2 * (uint64_t)r, windows);
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			done++;
		}
	}
	if (lane == 0) {
		if (done) atomicAdd(LONG ? &ctr->by_long : &ctr->by_lds, done);
		if (skipped) atomicAdd(&ctr->skipped, skipped);
		if (windows) atomicAdd(&ctr->windows, windows);
	}
}

// What the host loop of dbgk_map_reads finds out about offsets it holds, for offsets that lie on the device
// (dbgk_map_reads_device): chk[0] = the longest read, chk[1] = the number of reads whose offsets decrease, chk[2] = off[n_reads].
// A decreasing pair counts as a length of 2^64 - something, so chk[0] alone would refuse it too; chk[1] says why.
__global__ __launch_bounds__(256) void k_map_check_batch(const uint64_t *__restrict__ off, uint32_t n_reads, unsigned long long *__restrict__ chk)
{
	unsigned long long longest = 0, bad = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * 256) {
		const uint64_t a = off[i], b = off[i + 1];
		if (b < a) bad++;
		else longest = b - a > longest ? b - a : longest;
		if (i + 1 == n_reads) chk[2] = b;
	}
	for (int d = 32; d > 0; d >>= 1) {
		const unsigned long long o = __shfl_down(longest, d, 64);
		longest = o > longest ? o : longest;
		bad += __shfl_down(bad, d, 64);
	}
	if ((threadIdx.x & 63u) == 0u) {
		if (longest) atomicMax(&chk[0], longest);
		if (bad) atomicAdd(&chk[1], bad);
	}
}

} // namespace mapk
} // namespace dbgk
