// SIMPLIFY on 128-bit keys: the three kernels of dbgk_simplify.h that read k-mers, for tables of dbgk_node32 (k = 33..63).  PARITY
// UNPINNED above k = 32: the reference stops at k = 31; the rules are those of include/dbgk_wide.h and dbgk_wide_contig.h, each of which
// is the 64-bit rule when the high word is 0, so these kernels at k <= 31 on a table of {0, kmer} nodes give what k_simp_trace,
// k_simp_branches and k_simp_fill give (tests/test_simplify_gpu.py).  k_simp_update serves both kinds of table.
#pragma once

#include "dbgk_simplify.h"
#include "dbgk_wide_contig.h"

namespace wsimpk {

using dbgk_wide::Key128;
using simpk::kSimpThreads;
using simpk::Row;
using wctgk::WideTable;

struct Ops128 {
	using Tab = WideTable;
	using Key = Key128;
	static __device__ __forceinline__ Key key_at(const Tab &t, uint64_t slot) { return Key128{t.array[slot].kmer_hi, t.array[slot].kmer_lo}; }
	static __device__ __forceinline__ uint32_t link_at(const Tab &t, uint64_t slot, uint32_t left) { return left ? t.array[slot].l_link : t.array[slot].r_link; }
	static __device__ __forceinline__ bool same(const Tab &t, uint64_t slot, Key key)
	{
		return t.array[slot].kmer_lo == key.lo && t.array[slot].kmer_hi == key.hi;
	}
	static __device__ __forceinline__ Key neighbour(const Tab &t, Key kmer, uint32_t base, uint32_t left, bool &flip)
	{
		const Key nk = left ? wctgk::next_leftward(kmer, base, t.k) : wctgk::next_rightward(kmer, base, t.k);
		const Key rc = dbgk_wide::revcomp(nk, t.k);
		flip = dbgk_wide::less_equal(rc, nk);
		return flip ? rc : nk;
	}
	static __device__ __forceinline__ uint64_t hash(Key key) { return dbgk_wide::hash128(key); }
};

__global__ __launch_bounds__(kSimpThreads) void k_wsimp_trace(WideTable t, const uint32_t *__restrict__ req_slot, const int8_t *__restrict__ req_direct,
                                                              uint32_t n, int32_t cutoff, Row *__restrict__ rows)
{
	simpk::trace_body<Ops128>(t, req_slot, req_direct, n, cutoff, rows);
}

__global__ __launch_bounds__(kSimpThreads) void k_wsimp_branches(WideTable t, const uint32_t *__restrict__ slots, uint32_t n_rows, int32_t cutoff,
                                                                 int32_t freq_cutoff, Row *__restrict__ rows)
{
	simpk::branches_body<Ops128>(t, slots, n_rows, cutoff, freq_cutoff, rows);
}

__global__ __launch_bounds__(kSimpThreads) void k_wsimp_fill(WideTable t, const Row *__restrict__ rows, const uint64_t *__restrict__ first, uint32_t n,
                                                             int32_t cutoff, uint32_t *__restrict__ nodes, uint8_t *__restrict__ codes)
{
	simpk::fill_body<Ops128>(t, rows, first, n, cutoff, nodes, codes);
}

} // namespace wsimpk
