// The cleaner's length rule and offset checks (csrc/dbgk_clean_rule.h) as a plain program: built by tests/test_clean_compact_cpu.py
// with -fsanitize=address,undefined and run on the CPU.  Every record the kernels can write is compared with the loop of the two
// programs done on std::string (substr and all); records that point outside their read must keep nothing; the offset checks are
// walked over arrays of exactly the size they may touch, so that a read past n + 1 entries is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "dbgk_clean_rule.h"

using namespace dbgk::cleank;

static int g_checks = 0, g_bad = 0;

static void check(bool ok, const char *what, long a = 0, long b = 0, long c = 0)
{
	g_checks++;
	if (!ok) {
		g_bad++;
		printf("FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
	}
}

struct Tally {
	unsigned long long raw = 0, tr = 0, tb = 0, sr = 0, sb = 0, cr = 0, cb = 0;
};

static bool same(const CleanTally &t, const Tally &w)
{
	return t.raw_bases == w.raw && t.trimmed_reads == w.tr && t.trimmed_bases == w.tb && t.short_reads == w.sr && t.short_bases == w.sb &&
	       t.clean_reads == w.cr && t.clean_bases == w.cb;
}

// host/clean_lowqual.cpp:94-116 on a string of L bytes
static std::string lowqual_loop(const std::string &in, int start, int length, int trimmed, int min_len, Tally &w)
{
	std::string read = in;
	w.raw += in.size();
	if (trimmed) {
		read = start >= 1 ? read.substr(start - 1, length) : "";
		w.tr++;
		w.tb += in.size() - length;
	}
	if (read.size() < (size_t)min_len) {
		w.sr++;
		w.sb += read.size();
		read = "";
	}
	if (read.size()) {
		w.cr++;
		w.cb += read.size();
	}
	return read;
}

// host/clean_adapter.cpp:155-176
static std::string adapter_loop(const std::string &in, int adapter, int read_start, int min_len, Tally &w)
{
	std::string read = in;
	w.raw += in.size();
	if (adapter >= 0) {
		read = read.substr(0, read_start - 1);
		w.tr++;
		w.tb += in.size() - read_start + 1;
	}
	if (read.size() < (size_t)min_len) {
		w.sr++;
		w.sb += read.size();
		read = "";
	} else {
		w.cr++;
		w.cb += read.size();
	}
	return read;
}

int main()
{
	// every record a kernel can write for reads of 0 .. 12 bytes, at four values of -r
	for (int min_len : {0, 1, 5, 13}) {
		CleanTally t_low, t_ad;
		Tally w_low, w_ad;
		bool bytes_ok = true;
		for (int L = 0; L <= 12; ++L) {
			std::string in;
			for (int i = 0; i < L; ++i) in += (char)('a' + i);
			// clean_lowqual: untrimmed (start 1, or 0 for an empty read); trimmed with nothing kept; trimmed with a block inside the read
			std::vector<std::vector<int>> blocks = {{L ? 1 : 0, L, 0}, {0, 0, 1}};
			for (int s = 1; s <= L; ++s)
				for (int len = 1; s - 1 + len <= L; ++len) blocks.push_back({s, len, 1});
			for (const auto &b : blocks) {
				const CleanCut cut = clean_cut_lowqual((uint32_t)L, b[0], b[1], b[2]);
				const uint32_t m = t_low.add(DBGK_CLEAN_KIND_LOWQUAL, (uint32_t)L, cut, (uint32_t)min_len);
				const std::string want = lowqual_loop(in, b[0], b[1], b[2], min_len, w_low);
				bytes_ok = bytes_ok && cut.start + cut.len <= (uint32_t)L && (m ? in.substr(cut.start, m) : std::string()) == want;
			}
			// clean_adapter: no hit; a hit that starts at any byte of the read
			for (int rs = 0; rs <= L; ++rs) {
				const int adapter = rs ? 3 : -1;
				const CleanCut cut = clean_cut_adapter((uint32_t)L, adapter, rs);
				const uint32_t m = t_ad.add(DBGK_CLEAN_KIND_ADAPTER, (uint32_t)L, cut, (uint32_t)min_len);
				const std::string want = adapter_loop(in, adapter, rs, min_len, w_ad);
				bytes_ok = bytes_ok && cut.start == 0 && cut.len <= (uint32_t)L && in.substr(0, m) == want;
			}
		}
		check(bytes_ok, "kept bytes equal the programs' substr", min_len);
		check(same(t_low, w_low), "clean_lowqual's counters", min_len);
		check(same(t_ad, w_ad), "clean_adapter's counters", min_len);
	}
	// the two asymmetries, on one empty read with -r 0
	{
		CleanTally a, l;
		a.add(DBGK_CLEAN_KIND_ADAPTER, 0, clean_cut_adapter(0, -1, 0), 0);
		l.add(DBGK_CLEAN_KIND_LOWQUAL, 0, clean_cut_lowqual(0, 0, 0, 0), 0);
		check(a.clean_reads == 1 && l.clean_reads == 0 && a.short_reads == 0 && l.short_reads == 0, "an empty read is clean for clean_adapter only");
	}
	// records that point outside their read keep nothing and are still counted as trimmed
	const int32_t big = INT32_MAX, low = INT32_MIN;
	const int32_t outside_low[][2] = {{2, 10}, {11, 1}, {12, 0}, {1, 11}, {-1, 3}, {1, -1}, {big, big}, {big, 1}, {1, big}, {low, 1}, {1, low}, {low, low}};
	for (const auto &b : outside_low) {
		const CleanCut cut = clean_cut_lowqual(10, b[0], b[1], 1);
		check(cut.len == 0 && cut.start == 0 && cut.trimmed == 1, "lowqual block outside its read", b[0], b[1]);
	}
	check(clean_cut_lowqual(10, 11, 0, 1).len == 0 && clean_cut_lowqual(10, 11, 0, 1).start == 10, "an empty block behind the last byte is inside");
	check(clean_cut_lowqual(10, big, big, 0).len == 10, "an untrimmed read ignores start and length");
	const int32_t outside_ad[] = {12, 0, -1, big, low};
	for (int32_t rs : outside_ad) {
		const CleanCut cut = clean_cut_adapter(10, 0, rs);
		check(cut.len == 0 && cut.trimmed == 1, "adapter hit outside its read", rs);
	}
	check(clean_cut_adapter(10, 0, 11).len == 10 && clean_cut_adapter(10, 0, 1).len == 0, "read_start L + 1 keeps the read, 1 keeps nothing");
	check(clean_cut_adapter(10, -1, low).len == 10 && clean_cut_adapter(10, -1, low).trimmed == 0, "no hit ignores read_start");
	{
		const uint32_t top = (1u << 30) - 1; // the longest read a batch may hold
		check(clean_cut_lowqual(top, 1, (int32_t)top, 1).len == top && clean_cut_lowqual(top, 2, (int32_t)top, 1).len == 0, "longest read, lowqual");
		check(clean_cut_adapter(top, 0, (int32_t)top + 1).len == top && clean_cut_adapter(top, 0, big).len == 0, "longest read, adapter");
		CleanTally t;
		for (int i = 0; i < 8; ++i) t.add(DBGK_CLEAN_KIND_ADAPTER, top, clean_cut_adapter(top, -1, 0), 75);
		check(t.raw_bases == 8ull * top && t.clean_bases == 8ull * top, "64-bit sums");
	}
	// offset checks: arrays of exactly n + 1 entries
	{
		uint64_t max_len = 99;
		check(clean_check_batch(nullptr, 0, &max_len) == DBGK_ERR_ARG, "null offsets");
		std::vector<uint64_t> one = {0};
		check(clean_check_batch(one.data(), 0, &max_len) == DBGK_OK && max_len == 0, "no reads");
		one[0] = 1;
		check(clean_check_batch(one.data(), 0, &max_len) == DBGK_ERR_ARG, "offsets[0] != 0");
		std::vector<uint64_t> off = {0, 5, 5, 12};
		check(clean_check_batch(off.data(), 3, &max_len) == DBGK_OK && max_len == 7, "longest read");
		off[2] = 4;
		check(clean_check_batch(off.data(), 3, &max_len) == DBGK_ERR_ARG, "decreasing offsets");
		std::vector<uint64_t> lim = {0, (1ull << 30) - 1};
		check(clean_check_batch(lim.data(), 1, &max_len) == DBGK_OK, "a read of 2^30 - 1 bytes");
		lim[1] = 1ull << 30;
		check(clean_check_batch(lim.data(), 1, &max_len) == DBGK_ERR_ARG, "a read of 2^30 bytes");
		lim = {0, UINT64_MAX};
		check(clean_check_batch(lim.data(), 1, &max_len) == DBGK_ERR_ARG, "a read of 2^64 - 1 bytes");
		one[0] = 0;
		check(clean_check_batch(one.data(), 1ull << 31, &max_len) == DBGK_ERR_ARG, "2^31 reads are refused before any offset is read");
	}
	if (g_bad) return 1;
	printf("%d checks ok\n", g_checks);
	return 0;
}
