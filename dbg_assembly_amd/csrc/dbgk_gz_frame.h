// DEFLATE stage, framing (include/dbgk.h, GZ section).  HIP-free: the stage's kernels and host code, the writers of the bin/ programs
// and tests/gz_frame_test.cpp include it.  A member is a gzip member with BGZF's `BC` extra field:
//   18 bytes  1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 42 43 02 00 | BSIZE = total size - 1 (u16)
//   one deflate block with BFINAL set
//    8 bytes  CRC-32 and ISIZE of the piece, little-endian
// and a piece holds at most kGzPiece bytes, so that its stored form fits BSIZE.  The 28-byte end marker is the member of no bytes.
// CRC-32 arithmetic is in zlib's reflected form: bit 31 of a word is x^0, P = 0xEDB88320.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#ifndef DBGK_GZ_HD
#define DBGK_GZ_HD
#endif

namespace dbgk {
namespace gzf {

constexpr uint32_t kGzPiece = 65280;   // htslib's figure: 65280 + 18 + 5 + 8 < 65536
constexpr uint32_t kGzHead = 18, kGzTail = 8, kGzStoredHead = 5, kGzMarker = 28;
constexpr uint32_t kGzSlot = 65536;    // a member is built in a slot of this size
constexpr uint32_t kCrcPoly = 0xEDB88320u;

static const uint8_t kEndMarker[kGzMarker] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0,
                                              0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// the 18 header bytes of a member of `member_bytes` in all (19..65536)
inline void gz_write_head(uint8_t *out, uint32_t member_bytes)
{
	memcpy(out, kEndMarker, 16);
	out[16] = (uint8_t)((member_bytes - 1) & 0xFF);
	out[17] = (uint8_t)((member_bytes - 1) >> 8);
}

inline void gz_write_tail(uint8_t *out, uint32_t crc, uint32_t isize)
{
	for (int i = 0; i < 4; ++i) {
		out[i] = (uint8_t)(crc >> (8 * i));
		out[4 + i] = (uint8_t)(isize >> (8 * i));
	}
}

// a(x) b(x) mod P
DBGK_GZ_HD inline uint32_t gz_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) {
		if ((a >> (31 - i)) & 1u) p ^= b;
		b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
	}
	return p;
}

// x^(8 * 2^k) mod P for k = 0..31: what a CRC is multiplied by when 2^k bytes follow
struct GzPowers {
	uint32_t x8[32];
};

inline GzPowers gz_powers()
{
	GzPowers t;
	uint32_t p = 0x80000000u >> 8; // x^8
	for (int k = 0; k < 32; ++k) {
		t.x8[k] = p;
		p = gz_mulmod(p, p);
	}
	return t;
}

// x^(8 n) mod P
DBGK_GZ_HD inline uint32_t gz_x8n(const GzPowers &t, uint64_t n)
{
	uint32_t p = 0x80000000u;
	for (int k = 0; n; ++k, n >>= 1)
		if (n & 1u) p = gz_mulmod(p, t.x8[k & 31]);
	return p;
}

// CRC-32 of A B from the CRC-32 of A, of B and the length of B (< 2^32 bytes)
inline uint32_t gz_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
	static const GzPowers t = gz_powers();
	return gz_mulmod(crc_a, gz_x8n(t, len_b & 0xFFFFFFFFull)) ^ crc_b;
}

struct GzMember {
	uint64_t offset; // of the member in the buffer
	uint32_t size;   // all of it: BSIZE + 1
	uint32_t isize;  // bytes it inflates to
	uint32_t crc;
};

// The members of buf[0, n) by following BSIZE: up to `capacity` of them are written to `out` (may be null), *n_members counts all.
// Returns 0, or the reason the buffer is not this framing: 1 a member is cut short, 2 not the 16 fixed header bytes, 3 a BSIZE too
// small to hold header and trailer, 4 ISIZE above a piece.  *n_members then counts the whole members in front.  *n_markers (may be
// null) counts members with ISIZE 0 that are the end marker byte for byte.
inline int gz_frame_walk(const uint8_t *buf, uint64_t n, GzMember *out, uint64_t capacity, uint64_t *n_members, uint64_t *n_markers)
{
	uint64_t at = 0, count = 0, markers = 0;
	int rc = 0;
	while (at < n) {
		if (n - at < kGzHead + kGzTail + 2) { rc = 1; break; }
		if (memcmp(buf + at, kEndMarker, 16) != 0) { rc = 2; break; }
		const uint32_t size = ((uint32_t)buf[at + 16] | (uint32_t)buf[at + 17] << 8) + 1u;
		if (size < kGzHead + kGzTail + 2) { rc = 3; break; }
		if (n - at < size) { rc = 1; break; }
		const uint8_t *t = buf + at + size - kGzTail;
		GzMember m;
		m.offset = at;
		m.size = size;
		m.crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
		m.isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
		if (m.isize > kGzPiece) { rc = 4; break; }
		if (size == kGzMarker && memcmp(buf + at, kEndMarker, kGzMarker) == 0) markers++;
		if (out && count < capacity) out[count] = m;
		count++;
		at += size;
	}
	if (n_members) *n_members = count;
	if (n_markers) *n_markers = markers;
	return rc;
}

} // namespace gzf
} // namespace dbgk
