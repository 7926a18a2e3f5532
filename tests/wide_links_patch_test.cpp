// Stand-alone test of csrc/dbgk_wide_links_patch.h (no HIP, no GPU): the nodes a WIDE host table gets on the host after the device's
// link pass, patched into that pass's results.  Expected values come from a second, naive implementation below: records from a
// plain per-side scan, lists by appending and sorting.  Built with -fsanitize=address,undefined and run as a plain program by
// tests/test_wide_links_cpu.py; prints the number of cases and exits non-zero on the first difference.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dbgk_wide_links_patch.h"

using dbgk::PlacedNode;

static uint32_t word(int a, int c, int g, int t) { return (uint32_t)a << 24 | (uint32_t)c << 16 | (uint32_t)g << 8 | (uint32_t)t; } // A in bits 31..24
static uint64_t links(uint32_t l, uint32_t r) { return (uint64_t)l | (uint64_t)r << 32; }

struct Side {
	int num, base;
};

static Side naive_side(uint32_t w, int cutoff)
{
	const int d[4] = {(int)(w >> 24), (int)(w >> 16 & 255), (int)(w >> 8 & 255), (int)(w & 255)};
	Side s = {0, 0};
	int best = -1;
	for (int j = 0; j < 4; j++)
		if (d[j] > cutoff) s.num++;
	for (int j = 3; j >= 0; j--) // the first of equal largest counters wins: scan from the back, ties overwrite
		if (d[j] > cutoff && d[j] >= best) best = d[j], s.base = j;
	if (s.num > 3) s.num = 3;
	return s;
}

struct State {
	std::vector<uint16_t> klink;
	std::vector<uint8_t> del;
	std::vector<uint64_t> tips, branches; // whole buffers (capacity), the first nt / nb entries valid
	uint64_t nt, nb;
	dbgk_link_stats st;
};

static int n_cases = 0;

static void fail(const std::string &name, const char *what)
{
	fprintf(stderr, "case %s: %s differs\n", name.c_str(), what);
	exit(1);
}

// dev_tips / dev_branches: what the device pass listed (ascending); capacities of the two buffers; lists == false: counts only
static int run_case(const std::string &name, uint64_t size, std::vector<uint64_t> dev_tips, std::vector<uint64_t> dev_branches, const std::vector<PlacedNode> &placed,
                    int cutoff, uint64_t tip_cap, uint64_t branch_cap, bool lists = true, bool with_stats = true)
{
	n_cases++;
	State s;
	s.klink.assign(size, 0);
	s.del.assign(size / 8 + 1, 0);
	for (uint64_t v : dev_tips) s.klink[v] = 0x0001; // (some record of a tip: the patch must leave the device's records alone)
	for (uint64_t v : dev_branches) s.klink[v] = 0x0002;
	s.tips.assign(tip_cap + 1, 0xABABABABABABABABull); // one guard entry behind the capacity
	s.branches.assign(branch_cap + 1, 0xCDCDCDCDCDCDCDCDull);
	if (lists) {
		std::copy(dev_tips.begin(), dev_tips.end(), s.tips.begin());
		std::copy(dev_branches.begin(), dev_branches.end(), s.branches.begin());
	}
	s.nt = dev_tips.size();
	s.nb = dev_branches.size();
	memset(&s.st, 0, sizeof s.st);
	s.st.total_nodes = 1000, s.st.depth_stat[0] = 77, s.st.depth_stat[255] = 5, s.st.tip_nodes = (int64_t)s.nt, s.st.branch_nodes = (int64_t)s.nb;
	const State before = s;

	// the naive expectation
	State w = before;
	std::vector<uint64_t> want_tips = dev_tips, want_branches = dev_branches;
	for (const PlacedNode &p : placed) {
		const uint32_t l = (uint32_t)p.links, r = (uint32_t)(p.links >> 32);
		const Side a = naive_side(l, cutoff), b = naive_side(r, cutoff);
		w.klink[p.slot] = (uint16_t)(a.num | a.base << 2 | b.num << 4 | b.base << 6 | ((a.num == 1 && b.num == 1) ? 0x100 : 0));
		for (uint32_t x : {l, r})
			for (int sh = 0; sh < 32; sh += 8) w.st.depth_stat[x >> sh & 255]++;
		w.st.total_nodes++;
		if (a.num == 0 && b.num == 0) w.del[p.slot / 8] |= (uint8_t)(0x80 >> (p.slot % 8)), w.st.deleted_lowfreq++;
		if (a.num == 1 && b.num == 1) w.st.linear_nodes++;
		if (a.num + b.num == 1) want_tips.push_back(p.slot), w.st.tip_nodes++;
		if (a.num > 1 || b.num > 1) want_branches.push_back(p.slot), w.st.branch_nodes++;
	}
	std::sort(want_tips.begin(), want_tips.end());
	std::sort(want_branches.begin(), want_branches.end());
	const bool fits = !lists || (want_tips.size() <= tip_cap && want_branches.size() <= branch_cap);

	const int rc = dbgk::patch_placed_links(placed, cutoff, s.klink.data(), s.del.data(), lists ? s.tips.data() : nullptr, tip_cap, &s.nt,
	                                        lists ? s.branches.data() : nullptr, branch_cap, &s.nb, with_stats ? &s.st : nullptr);
	if (rc != (fits ? DBGK_OK : DBGK_ERR_CAPACITY)) fail(name, "status");
	if (s.nt != want_tips.size() || s.nb != want_branches.size()) fail(name, "counts");
	if (s.klink != w.klink) fail(name, "klink");
	if (s.del != w.del) fail(name, "del_flag");
	if (memcmp(&s.st, with_stats ? &w.st : &before.st, sizeof s.st)) fail(name, "stats");
	if (lists && fits) {
		if (!std::equal(want_tips.begin(), want_tips.end(), s.tips.begin())) fail(name, "tips");
		if (!std::equal(want_branches.begin(), want_branches.end(), s.branches.begin())) fail(name, "branches");
		if (!std::equal(s.tips.begin() + want_tips.size(), s.tips.end(), before.tips.begin() + want_tips.size())) fail(name, "tips behind the list");
		if (!std::equal(s.branches.begin() + want_branches.size(), s.branches.end(), before.branches.begin() + want_branches.size())) fail(name, "branches behind the list");
	} else if (s.tips != before.tips || s.branches != before.branches) {
		fail(name, "untouched lists");
	}
	return rc;
}

int main()
{
	const uint32_t none = word(0, 0, 0, 0), one = word(0, 9, 0, 0), two = word(4, 0, 0, 8);
	const uint64_t TIP = links(one, none), TIP_R = links(none, one), BRANCH = links(two, one), LINEAR = links(one, word(0, 0, 0, 3)), DELETED = links(word(2, 1, 0, 2), none);
	const std::vector<uint64_t> T = {10, 20, 30}, B = {11, 21, 31, 41};

	run_case("nothing placed", 64, T, B, {}, 2, 3, 4);
	run_case("empty lists", 64, {}, {}, {{5, TIP}, {6, BRANCH}}, 2, 1, 1);
	run_case("empty lists, empty table of 1 slot", 1, {}, {}, {{0, DELETED}}, 2, 0, 0);
	run_case("below every entry", 64, T, B, {{5, TIP}, {3, BRANCH}}, 2, 4, 5);
	run_case("above every entry", 64, T, B, {{63, TIP_R}, {50, BRANCH}}, 2, 4, 5);
	run_case("between two entries", 64, T, B, {{25, TIP}, {22, BRANCH}}, 2, 4, 5);
	run_case("below, between and above, given unsorted", 64, T, B, {{40, TIP}, {5, TIP}, {25, TIP_R}, {60, BRANCH}, {0, BRANCH}, {35, BRANCH}}, 2, 6, 7);
	run_case("two adjacent in one list", 64, T, B, {{22, TIP}, {23, TIP}, {12, BRANCH}, {13, BRANCH}}, 2, 5, 6);
	run_case("two adjacent at the front and the back", 64, T, B, {{1, TIP}, {2, TIP}, {62, BRANCH}, {63, BRANCH}}, 2, 5, 6);
	if (run_case("capacity exactly sufficient", 64, T, B, {{5, TIP}, {25, TIP}, {22, BRANCH}}, 2, 5, 5) != DBGK_OK) fail("capacity", "status");
	if (run_case("tip capacity one short", 64, T, B, {{5, TIP}, {25, TIP}, {22, BRANCH}}, 2, 4, 5) != DBGK_ERR_CAPACITY) fail("capacity", "status");
	if (run_case("branch capacity one short", 64, T, B, {{5, TIP}, {25, TIP}, {22, BRANCH}}, 2, 5, 4) != DBGK_ERR_CAPACITY) fail("capacity", "status");
	run_case("counts only", 64, T, B, {{5, TIP}, {22, BRANCH}}, 2, 0, 0, false);
	run_case("no stats", 64, T, B, {{5, TIP}, {22, BRANCH}}, 2, 4, 5, true, false);
	run_case("one of each class", 64, T, B, {{1, DELETED}, {2, LINEAR}, {3, TIP}, {4, BRANCH}, {9, TIP_R}}, 2, 5, 5);
	run_case("delete bits at both ends of a byte and in the last, partial byte", 21, {}, {}, {{0, DELETED}, {7, DELETED}, {8, DELETED}, {20, DELETED}}, 2, 0, 0);
	run_case("counters 0 and 255", 64, T, B, {{7, links(word(0, 255, 0, 255), word(255, 0, 0, 0))}, {8, links(none, none)}, {9, links(~0u, ~0u)}}, 2, 4, 7);
	run_case("counters at the cutoff and one above", 64, T, B, {{7, links(word(5, 6, 5, 0), word(5, 5, 5, 5))}}, 5, 4, 5);
	run_case("cutoff 0", 64, T, B, {{7, links(word(0, 1, 0, 0), word(0, 0, 0, 0))}, {8, links(word(1, 1, 0, 0), none)}}, 0, 4, 5);
	run_case("strongest-base tie", 64, T, B, {{7, links(word(0, 9, 9, 0), word(3, 200, 3, 200))}}, 2, 4, 5);
	run_case("four links on one side", 64, T, B, {{7, links(word(3, 4, 5, 6), none)}, {8, links(one, word(9, 9, 9, 9))}}, 2, 4, 6);

	// the last three once more against values written out by hand (independent of both implementations)
	{
		uint16_t klink[8] = {0};
		uint8_t del[2] = {0, 0};
		uint64_t nt = 0, nb = 0;
		const std::vector<PlacedNode> placed = {{1, links(word(0, 9, 9, 0), word(3, 200, 3, 200))}, {2, links(word(3, 4, 5, 6), none)}, {3, links(one, word(0, 0, 3, 0))}};
		if (dbgk::patch_placed_links(placed, 2, klink, del, nullptr, 0, &nt, nullptr, 0, &nb, nullptr) != DBGK_OK) fail("by hand", "status");
		// tie: 2 links, first of the two 9s = C (1) | right: 4 links capped at 3, first of the two 200s = C (1)
		if (klink[1] != (2 | 1 << 2 | 3 << 4 | 1 << 6)) fail("by hand", "tie record");
		if (klink[2] != (3 | 3 << 2)) fail("by hand", "four-link record");   // 3 links, strongest base T (3); nothing on the right
		if (klink[3] != (1 | 1 << 2 | 1 << 4 | 2 << 6 | 0x100)) fail("by hand", "linear record");
		if (nt != 0 || nb != 2 || del[0] != 0) fail("by hand", "counts");
		n_cases++;
	}
	printf("%d cases ok\n", n_cases);
	return 0;
}
