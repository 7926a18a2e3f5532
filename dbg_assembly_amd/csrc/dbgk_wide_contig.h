// CONTIG on 128-bit keys: the two kernels of the contig read-out that read k-mers, for tables of dbgk_node32 (k = 33..63; host side in
// dbgk_host_contig.h).  PARITY UNPINNED above k = 32: the reference stops at k = 31, the rules are those of include/dbgk_wide.h --
// revcomp, the 128-bit comparison, hash128, linear probing with wrap -- and with a high word of 0 every one of them is the 64-bit
// rule of dbgk_contig.h, so these kernels run at k <= 31 on a table of {0, kmer} nodes give what k_contig_successors and
// k_contig_emit give (tests/test_wide_contig_gpu.py).  The other eight kernels of dbgk_contig.h read flags, link records and port
// states only and serve both kinds of table unchanged.
#pragma once

#include "dbgk_contig.h"
#include "dbgk_wide.h"

namespace wctgk {

using contigk::END_ABSENT;
using contigk::END_BREAK_NODE;
using contigk::END_NONE;
using contigk::END_REPEAT;
using contigk::END_UNIQUE;
using contigk::kContigThreads;
using contigk::kEnd;
using contigk::Record;
using dbgk::ModMagic;
using dbgk_wide::Key128;

struct WideTable {
	const dbgk_node32 *array;
	const uint8_t *nul, *del;
	const uint16_t *klink;
	uint64_t size;
	ModMagic magic;
	int k;
};

__device__ __forceinline__ bool bit_of(const uint8_t *flags, uint64_t i) { return (flags[i >> 3] & (0x80u >> (i & 7u))) != 0; }

// the key's lowest 2 k bits, 1 <= k <= 63: the mask has 2 k - 64 bits in hi; at k = 32 it is all of lo and hi is empty
__device__ __forceinline__ Key128 head_mask(Key128 x, int k)
{
	const int bits = 2 * k;
	if (bits > 64) x.hi &= (1ull << (bits - 64)) - 1;
	else {
		x.hi = 0;
		if (bits < 64) x.lo &= (1ull << bits) - 1;
	}
	return x;
}

// contig.h:127-130 on 128 bits: two bits travel from lo up into hi
__device__ __forceinline__ Key128 next_rightward(Key128 x, uint32_t base, int k)
{
	return head_mask(Key128{(x.hi << 2) | (x.lo >> 62), (x.lo << 2) | base}, k);
}

// contig.h:119-123 on 128 bits: two bits travel from hi down into lo, the base lands at bit 2 (k - 1) -- in hi from k = 33 on
__device__ __forceinline__ Key128 next_leftward(Key128 x, uint32_t base, int k)
{
	Key128 r{x.hi >> 2, (x.lo >> 2) | (x.hi << 62)};
	const int sh = 2 * (k - 1);
	if (sh >= 64) r.hi += (uint64_t)base << (sh - 64);
	else r.lo += (uint64_t)base << sh;
	return r;
}

// base j (0 = first) of a k-base key
__device__ __forceinline__ uint32_t base_at(Key128 x, int k, uint32_t j)
{
	const uint32_t sh = 2u * ((uint32_t)k - 1u - j);
	return (uint32_t)(sh >= 64u ? x.hi >> (sh - 64u) : x.lo >> sh) & 3u;
}

// k_contig_successors on a table of 32-byte nodes: same outputs, same end classes.  The walk changes direction when the neighbour
// is not smaller than its reverse complement (contig.cpp:802: a palindrome counts as flipped; its key is the same either way).
__global__ __launch_bounds__(kContigThreads) void k_wctg_successors(WideTable t, const uint32_t *__restrict__ slot_of,
                                                                    const uint32_t *__restrict__ dense_of, uint32_t n_ports,
                                                                    uint32_t *__restrict__ raw_next, uint32_t *__restrict__ step,
                                                                    uint32_t *__restrict__ end_slot)
{
	for (uint32_t p = blockIdx.x * kContigThreads + threadIdx.x; p < n_ports; p += gridDim.x * kContigThreads) {
		const uint32_t left = p & 1u;
		const uint64_t u = slot_of[p >> 1];
		const Key128 self{t.array[u].kmer_hi, t.array[u].kmer_lo};
		const uint32_t kl = t.klink[u];
		const uint32_t base = left ? (kl >> 2) & 3u : (kl >> 6) & 3u;
		const uint32_t link = left ? t.array[u].l_link : t.array[u].r_link;
		const uint32_t depth = (link >> ((3u - base) * 8u)) & 0xffu;
		const Key128 nk = left ? next_leftward(self, base, t.k) : next_rightward(self, base, t.k);
		const Key128 rc = dbgk_wide::revcomp(nk, t.k);
		const bool flip = dbgk_wide::less_equal(rc, nk);
		const Key128 key = flip ? rc : nk;
		uint64_t v = dbgk::fast_mod(dbgk_wide::hash128(key), t.magic);
		bool found = false;
		for (uint64_t tries = 0; tries < t.size; ++tries) {            // a table without an empty slot ends here, not in a loop
			if (!bit_of(t.nul, v)) break;
			if (t.array[v].kmer_lo == key.lo && t.array[v].kmer_hi == key.hi) {
				found = !bit_of(t.del, v);
				break;
			}
			v = v + 1 == t.size ? 0 : v + 1;
		}
		uint32_t cls = END_ABSENT, nxt = kEnd, es = kEnd;
		if (found) {
			const uint32_t kv = t.klink[v];
			const uint32_t left_after = flip ? left ^ 1u : left;        // the walk's direction at the neighbour
			es = (uint32_t)v;
			if (kv & 0x100u) {
				cls = END_NONE;
				nxt = 2u * dense_of[v] + left_after;
			} else {
				const uint32_t vl = kv & 3u, vr = (kv >> 4) & 3u;
				if (vl == 0 || vr == 0) cls = END_BREAK_NODE;
				else cls = (left_after ? vl > 1 : vr > 1) ? END_REPEAT : END_UNIQUE;
			}
		}
		raw_next[p] = nxt;
		step[p] = base | (depth << 8) | (cls << 16);
		end_slot[p] = es;
	}
}

// k_contig_emit on a table of 32-byte nodes: the anchor's k bases come from both words of its key
__global__ __launch_bounds__(kContigThreads) void k_wctg_emit(const uint16_t *__restrict__ stage, const uint64_t *__restrict__ ctg_off,
                                                              const Record *__restrict__ rec, const dbgk_node32 *__restrict__ array,
                                                              uint32_t n_contigs, uint64_t total, int k, uint8_t *__restrict__ bases,
                                                              uint8_t *__restrict__ depths)
{
	const uint64_t n_words = (total + 7) / 8;
	for (uint64_t w = (uint64_t)blockIdx.x * kContigThreads + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * kContigThreads) {
		const uint64_t p0 = w * 8;
		uint32_t lo = 0, hi = n_contigs;                 // the contig with ctg_off[c] <= p0 < ctg_off[c + 1] (no contig is empty)
		while (hi - lo > 1) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (ctg_off[mid] <= p0) lo = mid; else hi = mid;
		}
		uint32_t c = lo;
		uint64_t c_begin = ctg_off[c], c_end = ctg_off[c + 1];
		uint32_t left_len = rec[c].left_len, md = rec[c].mid_depth;
		uint64_t anchor = rec[c].anchor;
		Key128 kmer{array[anchor].kmer_hi, array[anchor].kmer_lo};
		uint64_t wb = 0, wd = 0;
		const uint32_t n_bytes = (uint32_t)(total - p0 < 8 ? total - p0 : 8);
		for (uint32_t b = 0; b < n_bytes; ++b) {
			const uint64_t p = p0 + b;
			while (p >= c_end) {
				++c;
				c_begin = c_end;
				c_end = ctg_off[c + 1];
				left_len = rec[c].left_len;
				md = rec[c].mid_depth;
				anchor = rec[c].anchor;
				kmer = Key128{array[anchor].kmer_hi, array[anchor].kmer_lo};
			}
			const uint64_t rel = p - c_begin;
			uint32_t code, depth;
			if (rel >= left_len && rel < left_len + (uint32_t)k) {
				code = base_at(kmer, k, (uint32_t)(rel - left_len));
				depth = md;
			} else {
				const uint32_t s = stage[p];
				code = s & 3u;
				depth = s >> 8;
			}
			wb |= (uint64_t)((0x54474341u >> (8 * code)) & 0xffu) << (8 * b);   // "ACGT"
			wd |= (uint64_t)depth << (8 * b);
		}
		if (n_bytes == 8) {
			*reinterpret_cast<uint64_t *>(bases + p0) = wb;
			*reinterpret_cast<uint64_t *>(depths + p0) = wd;
		} else {
			for (uint32_t b = 0; b < n_bytes; ++b) {
				bases[p0 + b] = (uint8_t)(wb >> (8 * b));
				depths[p0 + b] = (uint8_t)(wd >> (8 * b));
			}
		}
	}
}

} // namespace wctgk
