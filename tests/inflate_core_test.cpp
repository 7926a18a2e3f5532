// The INFLATE stage's decode core (csrc/dbgk_inflate_core.h) as a host program, for the address and undefined-behaviour sanitizers:
//   inflate_core_test CASES [N_DAMAGED]
// CASES holds members, each behind its size as a little-endian u32.  Every member's stream is copied into a heap buffer of exactly its
// size, its tokens and bytes go to buffers of exactly ISIZE entries, so a read or write outside them is a sanitizer report.  Prints,
// per member, "verdict adler32 stored fixed dynamic literals matches largest-distance".  Then N_DAMAGED members with one byte or one bit changed (fixed
// seed) are decoded, and the count of loop iterations is checked against 8 * member bits + ISIZE.
#define DBGK_INF_COUNT_ITERATIONS 1
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "dbgk_gz_frame.h"
#include "dbgk_inflate_core.h"

using namespace dbgk;

static uint32_t adler32(const uint8_t *p, size_t n)
{
	uint32_t a = 1, b = 0;
	for (size_t i = 0; i < n; ++i) {
		a = (a + p[i]) % 65521u;
		b = (b + a) % 65521u;
	}
	return b << 16 | a;
}

struct Result {
	uint32_t reason = 0, adler = 1, isize = 0, max_dist = 0;
	inf::InfCount count{};
};

// what k_inf_resolve computes, one byte at a time: tokens -> out[0, isize) and their CRC-32.  false: a token reaches outside, which
// the decoder must have refused
static bool resolve_serial(const uint32_t *tok, uint32_t n_tok, uint8_t *out, uint32_t isize, uint32_t *crc_out, uint32_t *max_dist)
{
	uint32_t at = 0, crc = 0xFFFFFFFFu;
	for (uint32_t t = 0; t < n_tok; ++t) {
		const uint32_t k = tok[t];
		const bool match = (k >> 31) != 0;
		const uint32_t len = match ? ((k >> 15) & 0xFFu) + 3u : 1u, dist = (k & 0x7FFFu) + 1u;
		if (len > isize - at || (match && dist > at)) return false;
		if (match && dist > *max_dist) *max_dist = dist;
		for (uint32_t i = 0; i < len; ++i, ++at) {
			const uint8_t v = match ? out[at - dist] : (uint8_t)k;
			out[at] = v;
			crc ^= v;
			for (int j = 0; j < 8; ++j) crc = (crc >> 1) ^ (gzf::kCrcPoly & (0u - (crc & 1u)));
		}
	}
	*crc_out = ~crc;
	return at == isize;
}

static Result run_member(const uint8_t *m, uint32_t size)
{
	Result r;
	uint32_t crc = 0;
	r.reason = inf::inf_frame(m, size, &r.isize, &crc);
	// the walk of one member agrees with the frame check
	uint64_t n_members = 0;
	const int rc = gzf::gz_frame_walk(m, size, nullptr, 0, &n_members, nullptr);
	if ((rc == 0 && n_members == 1) != (r.reason == inf::R_OK)) {
		fprintf(stderr, "gz_frame_walk and inf_frame disagree\n");
		exit(2);
	}
	if (r.reason) return r;
	const uint32_t n = size - gzf::kGzHead - gzf::kGzTail;
	std::unique_ptr<uint8_t[]> stream(new uint8_t[n]);
	memcpy(stream.get(), m + gzf::kGzHead, n);
	std::unique_ptr<uint32_t[]> tok(new uint32_t[r.isize]);
	std::unique_ptr<uint8_t[]> out(new uint8_t[r.isize]);
	std::unique_ptr<inf::InfTables> T(new inf::InfTables);
	uint32_t n_tok = 0;
	r.reason = inf::inf_decode(stream.get(), n, r.isize, tok.get(), *T, &n_tok, r.count);
	if (r.reason) return r;
	uint32_t found = 0;
	if (!resolve_serial(tok.get(), n_tok, out.get(), r.isize, &found, &r.max_dist)) {
		fprintf(stderr, "the decoder accepted tokens that reach outside the member's bytes\n");
		exit(2);
	}
	if (found != crc) {
		r.reason = inf::R_CRC;
		return r;
	}
	r.adler = adler32(out.get(), r.isize);
	return r;
}

int main(int argc, char **argv)
{
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	std::vector<std::vector<uint8_t>> members;
	for (;;) {
		uint8_t s[4];
		if (fread(s, 1, 4, f) != 4) break;
		const uint32_t size = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
		std::vector<uint8_t> m(size);
		if (size && fread(m.data(), 1, size, f) != size) return 2;
		members.push_back(std::move(m));
	}
	fclose(f);
	for (const auto &m : members) {
		const Result r = run_member(m.data(), (uint32_t)m.size());
		printf("%u %u %u %u %u %u %u %u\n", r.reason, r.adler, r.count.n_stored, r.count.n_fixed, r.count.n_dynamic, r.count.n_literals, r.count.n_matches,
		       r.max_dist);
	}
	const long n_damaged = argc > 2 ? atol(argv[2]) : 0;
	uint64_t x = 0x9E3779B97F4A7C15ull, refused = 0, worst_num = 0, worst_den = 1;
	auto rnd = [&x]() {
		x ^= x << 13;
		x ^= x >> 7;
		x ^= x << 17;
		return x;
	};
	for (long i = 0; i < n_damaged && !members.empty(); ++i) {
		std::vector<uint8_t> m = members[(size_t)(rnd() % members.size())];
		if (m.empty()) continue;
		const size_t at = (size_t)(rnd() % m.size());
		if (i & 1) m[at] ^= (uint8_t)(1u << (rnd() % 8));
		else m[at] = (uint8_t)rnd();
		const Result r = run_member(m.data(), (uint32_t)m.size());
		const uint64_t bound = 8ull * 8ull * m.size() + r.isize;
		if (r.count.iterations > bound) {
			fprintf(stderr, "damaged member %ld: %llu iterations, bound %llu\n", i, (unsigned long long)r.count.iterations, (unsigned long long)bound);
			return 1;
		}
		if (r.count.iterations * worst_den > worst_num * bound) worst_num = r.count.iterations, worst_den = bound;
		refused += r.reason != 0;
	}
	printf("damaged %ld refused %llu worst %llu of %llu\n", n_damaged, (unsigned long long)refused, (unsigned long long)worst_num, (unsigned long long)worst_den);
	return 0;
}
