// dbgk_link_record.h -- the 2-byte KmerLink record of one node (DBG_contig/contig.h:31-42) from its two link words: ONE source for
// the device kernels (k_kmer_links, k_wide_kmer_links) and for host code that has no HIP (dbgk_wide_links_patch.h and its test).
// Needs <cstdint> only; DBGK_HD is `__host__ __device__` in the HIP translation unit and empty elsewhere.
#pragma once

#include <cstdint>

#ifndef DBGK_HD
#define DBGK_HD
#endif

namespace dbgk {

// links = l_link | r_link << 32
static inline __attribute__((always_inline)) DBGK_HD uint32_t kmer_link_record(uint64_t links, int cutoff)
{
	// contig.cpp:129-163: a side's link number = counters above the cutoff (at most 3: a 2-bit field), its base = the FIRST
	// base with the largest such counter (strict <), 0 when there is none
	uint32_t rec = 0;
#ifdef __HIP__
#pragma unroll
#endif
	for (int side = 0; side < 2; side++) {
		const uint32_t w = side ? (uint32_t)(links >> 32) : (uint32_t)links;
		int num = 0, best = 0, base = 0;
#ifdef __HIP__
#pragma unroll
#endif
		for (int j = 0; j < 4; j++) {
			const int d = (int)((w >> (24 - 8 * j)) & 0xFFu); // get_next_kmer_depth (kmerSet.cpp:341-344): A in bits 31..24
			if (d > cutoff) {
				if (num < 3) num++;
				if (best < d) { best = d; base = j; }
			}
		}
		rec |= ((uint32_t)num | ((uint32_t)base << 2)) << (4 * side);
	}
	if ((rec & 3u) == 1u && ((rec >> 4) & 3u) == 1u) rec |= 1u << 8; // linear: exactly one link on each side (:170-173)
	return rec;
}

} // namespace dbgk
