// dbgk_wide_links_patch.h -- the first pass of the contig stage (calculate_kmer_links, DBG_contig/contig.cpp:107-181) for the few
// nodes of a WIDE table that live outside the device table: keys with a zero low word (side table, at most 4096) and the key-0
// node.  dbgk_wide_export_host_table puts them on their probe chains on the host, after the image has left the device, so
// k_wide_kmer_links saw their final slots as empty.  patch_placed_links adds what the kernel would have written for them: the
// record, the delete bit, the eight counters and the class, and the slot at its ascending position in the tip / branch list.
//
// No HIP here (<cstdint>, <vector>, <algorithm> and the dbgk.h types): compiled on its own by tests/wide_links_patch_test.cpp.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "dbgk.h"
#include "dbgk_link_record.h"

namespace dbgk {

struct PlacedNode {
	uint64_t slot;  // where the host put it
	uint64_t links; // l_link | r_link << 32
};

// list[0, n) ascending, add ascending, room for n + add.size(): one merge from the back, in place
inline void merge_placed_slots(uint64_t *list, uint64_t n, const std::vector<uint64_t> &add)
{
	uint64_t w = n + add.size(), i = n;
	for (size_t j = add.size(); j > 0; j--) {
		while (i > 0 && list[i - 1] > add[j - 1]) list[--w] = list[--i];
		list[--w] = add[j - 1];
	}
}

// On entry klink / del_flag / stats / the lists and *n_tips / *n_branches are what the device pass left for the table without the
// placed nodes.  tip_nodes / branch_nodes / stats may be null (counts only / no stats).  Records, delete bits, stats and the two
// counts are always completed; DBGK_ERR_CAPACITY when a list cannot take its placed slots (*n_tips / *n_branches say what is
// needed, both lists are left as they were).
inline int patch_placed_links(const std::vector<PlacedNode> &placed, int32_t cutoff, uint16_t *klink, uint8_t *del_flag, uint64_t *tip_nodes,
                              uint64_t tip_capacity, uint64_t *n_tips, uint64_t *branch_nodes, uint64_t branch_capacity, uint64_t *n_branches,
                              dbgk_link_stats *stats)
{
	std::vector<uint64_t> tips, branches;
	for (const PlacedNode &p : placed) {
		const uint32_t rec = kmer_link_record(p.links, cutoff);
		const uint32_t ln = rec & 3u, rn = (rec >> 4) & 3u;
		klink[p.slot] = (uint16_t)rec;
		if (ln == 0u && rn == 0u) del_flag[p.slot >> 3] |= (uint8_t)(128u >> (p.slot & 7u));
		if (ln + rn == 1u) tips.push_back(p.slot);
		if (ln > 1u || rn > 1u) branches.push_back(p.slot);
		if (stats) {
			for (int b = 0; b < 8; b++) stats->depth_stat[(p.links >> (8 * b)) & 0xFFu]++;
			stats->total_nodes++;
			if (ln == 0u && rn == 0u) stats->deleted_lowfreq++;
			if (ln == 1u && rn == 1u) stats->linear_nodes++;
			if (ln + rn == 1u) stats->tip_nodes++;
			if (ln > 1u || rn > 1u) stats->branch_nodes++;
		}
	}
	std::sort(tips.begin(), tips.end());
	std::sort(branches.begin(), branches.end());
	const uint64_t nt = *n_tips, nb = *n_branches;
	*n_tips = nt + tips.size();
	*n_branches = nb + branches.size();
	if ((tip_nodes && *n_tips > tip_capacity) || (branch_nodes && *n_branches > branch_capacity)) return DBGK_ERR_CAPACITY;
	if (tip_nodes) merge_placed_slots(tip_nodes, nt, tips);
	if (branch_nodes) merge_placed_slots(branch_nodes, nb, branches);
	return DBGK_OK;
}

} // namespace dbgk
