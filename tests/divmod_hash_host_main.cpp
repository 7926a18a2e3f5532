// Stand-alone host program for tests/test_divmod_hash_host.py: the host-callable functions of dbgk_device.h on the CPU.
//   divmod_hash_host_main hash              u64 keys on stdin, one per line -> hash_code(key), one per line
//   divmod_hash_host_main div D [D ...]     divmod_magic_small against 128-bit division for every divisor D: the edge values
//                                           q d - 1, q d, q d + d - 1 for a spread of q, 0, 2^64 - 1, and 10^6 random h;
//                                           prints "D checked mismatches" per divisor, exit status 1 on any mismatch
// Built by the test with the HIP compiler (the header includes the HIP runtime's declarations), host side under ASan + UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dbgk_device.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t next_u64()
{
	rng_state += 0x9E3779B97F4A7C15ull;
	return dbgk::mix64(rng_state);
}

static uint64_t check_one(uint64_t h, const dbgk::ModMagic &g, uint64_t &bad)
{
	uint64_t q = 0;
	const uint32_t r = dbgk::divmod_magic_small(h, g.m, (uint32_t)g.d, q);
	const unsigned __int128 H = h;
	const uint64_t q_ref = (uint64_t)(H / g.d), r_ref = (uint64_t)(H % g.d);
	if (q != q_ref || r != r_ref) {
		if (bad < 5) printf("# d=%" PRIu64 " h=%" PRIu64 ": q=%" PRIu64 " r=%u, want q=%" PRIu64 " r=%" PRIu64 "\n", g.d, h, q, r, q_ref, r_ref);
		bad++;
	}
	return 1;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "hash")) {
		char line[64];
		while (fgets(line, sizeof line, stdin)) printf("%" PRIu64 "\n", dbgk::hash_code(strtoull(line, nullptr, 10)));
		return 0;
	}
	if (argc >= 3 && !strcmp(argv[1], "div")) {
		uint64_t bad_total = 0;
		for (int a = 2; a < argc; a++) {
			const uint64_t d = strtoull(argv[a], nullptr, 10);
			if (d < 2 || d >= (1ull << 31)) return 2;
			const dbgk::ModMagic g = dbgk::make_mod_magic(d);
			const uint64_t q_max = ~0ull / d;
			uint64_t n = 0, bad = 0;
			n += check_one(0ull, g, bad);
			n += check_one(~0ull, g, bad);
			// multiples of d and their neighbours: small q, q around 2^32 (the quotient's low word wraps), the largest q, random q
			uint64_t qs[64];
			int nq = 0;
			const uint64_t fixed[] = {1, 2, 3, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, (1ull << 33) - 1, q_max - 1, q_max};
			for (uint64_t q : fixed) qs[nq++] = q;
			while (nq < 64) qs[nq++] = 1 + next_u64() % q_max;
			for (int i = 0; i < nq; i++) {
				const uint64_t base = qs[i] * d; // (q <= q_max: no overflow)
				n += check_one(base - 1, g, bad);
				n += check_one(base, g, bad);
				if (base <= ~0ull - (d - 1)) n += check_one(base + d - 1, g, bad);
			}
			for (int i = 0; i < 1000000; i++) n += check_one(next_u64(), g, bad);
			printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", d, n, bad);
			bad_total += bad;
		}
		return bad_total ? 1 : 0;
	}
	fprintf(stderr, "usage: %s hash | div D [D ...]\n", argv[0]);
	return 2;
}
