// csrc/dbgk_gz_frame.h on its own: the member walk over good, truncated and mis-sized buffers, the header and trailer writers, and
// the CRC combine against zlib's crc32.  A program with its own main, built by tests/test_deflate_cpu.py with the system compiler
// and the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <zlib.h>

#include "dbgk_gz_frame.h"

using namespace dbgk::gzf;

static int n_cases = 0;
#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond)) {                                                     \
			printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
			return 1;                                                      \
		}                                                                  \
		n_cases++;                                                         \
	} while (0)

// a member with a stored block around `piece`
static void append_member(std::vector<uint8_t> &buf, const std::vector<uint8_t> &piece)
{
	const uint32_t n = (uint32_t)piece.size(), size = kGzHead + kGzStoredHead + n + kGzTail;
	const size_t at = buf.size();
	buf.resize(at + size);
	gz_write_head(&buf[at], size);
	uint8_t *p = &buf[at + kGzHead];
	p[0] = 1, p[1] = (uint8_t)n, p[2] = (uint8_t)(n >> 8), p[3] = (uint8_t)~n, p[4] = (uint8_t)(~n >> 8);
	for (uint32_t i = 0; i < n; ++i) p[5 + i] = piece[i];
	gz_write_tail(&buf[at + size - kGzTail], (uint32_t)crc32(0, piece.data(), n), n);
}

int main()
{
	std::vector<std::vector<uint8_t>> pieces;
	uint32_t seed = 12345;
	for (uint32_t n : {1u, 2u, 3u, 255u, 4096u, kGzPiece - 1, kGzPiece, 77u}) {
		std::vector<uint8_t> p(n);
		for (auto &b : p) b = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
		pieces.push_back(p);
	}
	std::vector<uint8_t> buf, all;
	std::vector<uint64_t> offsets;
	for (auto &p : pieces) {
		offsets.push_back(buf.size());
		append_member(buf, p);
		all.insert(all.end(), p.begin(), p.end());
	}
	const size_t marker_at = buf.size();
	buf.insert(buf.end(), kEndMarker, kEndMarker + kGzMarker);

	// ---- the walk over a good buffer
	std::vector<GzMember> ms(pieces.size() + 1);
	uint64_t n = 0, markers = 0;
	CHECK(gz_frame_walk(buf.data(), buf.size(), ms.data(), ms.size(), &n, &markers) == 0);
	CHECK(n == pieces.size() + 1 && markers == 1);
	for (size_t i = 0; i < pieces.size(); ++i) {
		CHECK(ms[i].offset == offsets[i] && ms[i].isize == pieces[i].size() && ms[i].size == pieces[i].size() + 31);
		CHECK(ms[i].crc == crc32(0, pieces[i].data(), (uInt)pieces[i].size()));
	}
	CHECK(ms[pieces.size()].offset == marker_at && ms[pieces.size()].size == kGzMarker && ms[pieces.size()].isize == 0);
	// counting only: no array, and an array too small
	CHECK(gz_frame_walk(buf.data(), buf.size(), nullptr, 0, &n, nullptr) == 0 && n == pieces.size() + 1);
	GzMember two[2];
	CHECK(gz_frame_walk(buf.data(), buf.size(), two, 2, &n, &markers) == 0 && n == pieces.size() + 1 && two[1].offset == offsets[1]);
	CHECK(gz_frame_walk(buf.data(), 0, nullptr, 0, &n, &markers) == 0 && n == 0 && markers == 0);
	CHECK(gz_frame_walk(kEndMarker, kGzMarker, two, 2, &n, &markers) == 0 && n == 1 && markers == 1);
	// the largest member fills BSIZE's range but for the bytes a piece leaves
	CHECK(ms[6].size == kGzPiece + 31 && ms[6].size <= kGzSlot);

	// ---- truncated: every cut inside the first two members and inside the marker
	for (size_t cut = 1; cut < offsets[2]; ++cut) {
		std::vector<uint8_t> part(buf.begin(), buf.begin() + cut); // (its own allocation: a read past the cut is an error of the sanitizer's)
		const int rc = gz_frame_walk(part.data(), part.size(), two, 2, &n, nullptr);
		if (cut == offsets[1]) CHECK(rc == 0 && n == 1);
		else CHECK(rc == 1 && n == (cut > offsets[1] ? 1u : 0u));
	}
	for (size_t cut = marker_at + 1; cut < buf.size(); ++cut) {
		std::vector<uint8_t> part(buf.begin(), buf.begin() + cut);
		CHECK(gz_frame_walk(part.data(), part.size(), nullptr, 0, &n, &markers) == 1 && n == pieces.size() && markers == 0);
	}
	// ---- a wrong BSIZE: one more and one less lead the walk off the next header; too small to be a member; a foreign header
	for (int delta : {-1, 1}) {
		std::vector<uint8_t> bad(buf);
		const uint32_t s = ms[3].size - 1 + delta;
		bad[offsets[3] + 16] = (uint8_t)s, bad[offsets[3] + 17] = (uint8_t)(s >> 8);
		CHECK(gz_frame_walk(bad.data(), bad.size(), nullptr, 0, &n, nullptr) != 0 && n <= 4);
	}
	{
		std::vector<uint8_t> bad(buf);
		bad[offsets[0] + 16] = 20, bad[offsets[0] + 17] = 0;
		CHECK(gz_frame_walk(bad.data(), bad.size(), nullptr, 0, &n, nullptr) == 3 && n == 0);
		bad = buf;
		bad[offsets[1] + 3] = 0; // FLG without FEXTRA: a plain gzip member
		CHECK(gz_frame_walk(bad.data(), bad.size(), nullptr, 0, &n, nullptr) == 2 && n == 1);
		bad = buf;
		bad[offsets[2] - 1] = 0xff; // ISIZE of member 1 above a piece
		CHECK(gz_frame_walk(bad.data(), bad.size(), nullptr, 0, &n, nullptr) == 4 && n == 1);
	}

	// ---- CRC: the powers, and the combine over the pieces in order against zlib's crc32 of the whole text
	CHECK(gz_mulmod(0x80000000u, 0x12345678u) == 0x12345678u);
	const GzPowers t = gz_powers();
	CHECK(t.x8[0] == 0x00800000u && gz_x8n(t, 0) == 0x80000000u && gz_x8n(t, 4) == kCrcPoly); // x^32 = P's low terms
	uint32_t crc = 0;
	uint64_t len = 0;
	for (auto &p : pieces) {
		crc = gz_crc_combine(crc, (uint32_t)crc32(0, p.data(), (uInt)p.size()), p.size());
		len += p.size();
		CHECK(crc == crc32(0, all.data(), (uInt)len));
	}
	CHECK(gz_crc_combine(crc, 0, 0) == crc);
	for (uint64_t zeros : {1ull, 255ull, 65280ull, (1ull << 20) + 3}) {
		std::vector<uint8_t> z(zeros, 0), both(all);
		both.insert(both.end(), z.begin(), z.end());
		CHECK(gz_crc_combine(crc, (uint32_t)crc32(0, z.data(), (uInt)zeros), zeros) == crc32(0, both.data(), (uInt)both.size()));
	}
	printf("%d cases ok\n", n_cases);
	return 0;
}
