// dbgk_clean_rule.h -- CLEAN, output stage: what a record makes of its read, and the numbers of the .stat file.  No HIP in here: the
// length kernel (dbgk_emit.h) and the host's argument checks (dbgk_host_clean.h) share it, and tests/clean_rule_test.cpp
// runs it as a plain program under the address and undefined-behaviour sanitizers.
//
// The rule is the loop of the two programs (host/clean_lowqual.cpp:85-117, host/clean_adapter.cpp:152-177) with one addition: a
// record that points outside its read -- the kernels write none, dbgk_clean_compact_from may be handed one -- keeps nothing, where
// std::string::substr would clamp or throw.  So no byte outside a read is ever copied.
#pragma once

#include <stdint.h>

#include "dbgk.h"

#if defined(__HIPCC__)
#define DBGK_CLEAN_HD __host__ __device__ __forceinline__
#else
#define DBGK_CLEAN_HD inline
#endif

namespace dbgk {
namespace cleank {

// what is kept of a read of L bytes before the short-read filter: bytes [start, start + len) of the read, 0-based
struct CleanCut {
	uint32_t start, len;
	uint32_t trimmed; // counted as trimmed by the program (TrimLowQual / Aligned to adapter)
};

// L < 2^30 (clean_check_batch)
DBGK_CLEAN_HD CleanCut clean_cut_lowqual(uint32_t L, int32_t start, int32_t length, int32_t trimmed)
{
	if (!trimmed) return CleanCut{0u, L, 0u};
	if (start < 1 || length < 0) return CleanCut{0u, 0u, 1u}; // start == 0: nothing is kept
	const uint64_t s = (uint64_t)start - 1u;
	if (s + (uint64_t)length > L) return CleanCut{0u, 0u, 1u};
	return CleanCut{(uint32_t)s, (uint32_t)length, 1u};
}

DBGK_CLEAN_HD CleanCut clean_cut_adapter(uint32_t L, int32_t adapter, int32_t read_start)
{
	if (adapter < 0) return CleanCut{0u, L, 0u};
	if (read_start < 1 || (uint64_t)read_start - 1u > L) return CleanCut{0u, 0u, 1u};
	return CleanCut{0u, (uint32_t)read_start - 1u, 1u};
}

// the integer columns of the .stat file but the first (the number of reads)
struct CleanTally {
	unsigned long long raw_bases = 0, trimmed_reads = 0, trimmed_bases = 0, short_reads = 0, short_bases = 0, clean_reads = 0, clean_bases = 0;

	// one read -> the length of its result.  The two asymmetries are the programs' own: clean_adapter counts every read that is not
	// short as clean (an empty one too when min_len is 0), clean_lowqual only a read that holds bytes.
	DBGK_CLEAN_HD uint32_t add(int32_t kind, uint32_t L, const CleanCut &cut, uint32_t min_len)
	{
		raw_bases += L;
		if (cut.trimmed) {
			trimmed_reads++;
			trimmed_bases += L - cut.len;
		}
		const bool is_short = cut.len < min_len;
		const uint32_t m = is_short ? 0u : cut.len;
		if (is_short) {
			short_reads++;
			short_bases += cut.len;
		}
		if (kind == DBGK_CLEAN_KIND_ADAPTER ? !is_short : m > 0u) {
			clean_reads++;
			clean_bases += m;
		}
		return m;
	}
};

// the checks every call makes on a batch's offsets; *max_len is the longest read
inline int clean_check_batch(const uint64_t *offsets, uint64_t n_reads, uint64_t *max_len)
{
	if (!offsets || offsets[0] != 0 || n_reads >= (1ull << 31)) return DBGK_ERR_ARG;
	*max_len = 0;
	for (uint64_t i = 0; i < n_reads; ++i) {
		if (offsets[i + 1] < offsets[i]) return DBGK_ERR_ARG;
		const uint64_t len = offsets[i + 1] - offsets[i];
		if (len > *max_len) *max_len = len;
	}
	return *max_len >= (1ull << 30) ? DBGK_ERR_ARG : DBGK_OK;
}

} // namespace cleank
} // namespace dbgk
