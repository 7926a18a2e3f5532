// Stand-alone check of csrc/dbgk_maprow_rule.h (built and run by tests/test_maprow_cpu.py under ASan / UBSan): the rule's text of
// the identity field against what the host loop prints, `ostream << float`, for the same (mismatches, align_len).  Prints nothing
// and exits 0 when every pair agrees; a pair the stream prints in exponent form, or as no number at all, must come back unprintable.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>

#include "dbgk_maprow_rule.h"

using namespace dbgk::maprule;

static long failures = 0;
static long printable = 0, unprintable = 0;

static std::string text_of(const IdentText &t)
{
	std::string s;
	for (uint32_t i = 0; i < t.n; ++i) s += (char)((i < 8 ? t.lo >> (8 * i) : t.hi >> (8 * (i - 8))) & 0xFF);
	return s;
}

static void check(int32_t m, int32_t a)
{
	// Contigs::row, word for word
	float identity = 1.0 - (float)m / a;
	std::ostringstream o;
	o << identity * 100;
	const std::string want = o.str();
	const bool plain = want.find_first_not_of("0123456789.") == std::string::npos;
	const IdentText t = ident_text(ident_value((float)m / (float)a));
	const std::string got = text_of(t);
	if (t.n > kIdentMax || (plain ? got != want : t.n != 0)) {
		if (failures++ < 20) fprintf(stderr, "m = %d, a = %d: the stream prints '%s', the rule '%s'\n", m, a, want.c_str(), got.c_str());
	}
	(plain ? printable : unprintable)++;
}

int main(int argc, char **argv)
{
	for (int32_t a = 0; a <= 4096; ++a)
		for (int32_t m = 0; m <= a; ++m) check(m, a);
	const long small_unprintable = unprintable; // 0 / 0 alone
	const int32_t big = 0x7FFFFFFF;
	check(1, 1 << 24);                 // 1 - 2^-24 rounds to 1: prints 100
	if (text_of(ident_text(ident_value(1.0f / (float)(1 << 24)))) != "100") failures++;
	const int32_t lens[] = {4097, 9999, 10000, 65535, 99999, 100000, 999983, 1000000, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 1, 1 << 24,
	                        (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, 20000003, 1 << 25, (1 << 25) + 5, 123456789, 1 << 30, (1 << 30) + 1, big - 1, big};
	for (int32_t a : lens) {
		const int32_t ms[] = {0, 1, 2, 3, 7, 10, 99, 1000, a / 1000, a / 100, a / 3, a / 2, a / 2 + 1, a - a / 7, a - 100000, a - 10001, a - 1000, a - 257,
		                      a - 100, a - 65, a - 64, a - 33, a - 10, a - 9, a - 5, a - 4, a - 3, a - 2, a - 1, a};
		for (int32_t m : ms)
			if (m >= 0 && m <= a) check(m, a);
	}
	// a pseudo-random sweep, half of it with m close to a (the small identities, where the exponent form begins)
	uint64_t x = 0x9E3779B97F4A7C15ull;
	auto next = [&]() {
		x ^= x << 13;
		x ^= x >> 7;
		x ^= x << 17;
		return x;
	};
	for (int i = 0; i < 200000; ++i) {
		const int32_t a = (int32_t)(next() % (uint64_t)big) + 1;
		const int32_t m = (i & 1) ? (int32_t)(next() % ((uint64_t)a + 1)) : a - (int32_t)(next() % (uint64_t)(a < 300 ? a + 1 : 300));
		check(m, a);
	}
	if (small_unprintable != 1 || unprintable - small_unprintable < 10 || printable < 8000000) {
		fprintf(stderr, "coverage: %ld printable, %ld unprintable, %ld of them up to 4096\n", printable, unprintable, small_unprintable);
		failures++;
	}
	if (argc > 1) printf("%ld printable, %ld unprintable\n", printable, unprintable); // (any argument: the counts, for a person)
	(void)argv;
	return failures ? 1 : 0;
}
