// INFLATE stage, the decode core (include/dbgk.h, INFLATE section; kernels in dbgk_inflate.h).  HIP-free, as dbgk_gz_frame.h is: the
// decode kernel and tests/inflate_core_test.cpp compile the same functions, so that the two rules below are checked on the host under
// the address and undefined-behaviour sanitizers before a corrupt member is ever sent to a device.
//   1. No byte outside the member is read, and no token outside the member's token area is written: every access is checked before
//      it is made.  The bit reader hands out zeros behind the stream's end and says so; a token is written only while the bytes of
//      all tokens stay within ISIZE, and as every token stands for at least one byte the area needs ISIZE entries.
//   2. Every data-driven loop consumes at least one bit or emits one token per iteration, or ends with a reason code.  The loops
//      over a code's lengths and tables have fixed bounds.
// A member's deflate stream (RFC 1951: stored, fixed and dynamic blocks, any number of them) becomes tokens in the deflater's form: a
// literal byte, or bit 31 | (length - 3) << 15 | (distance - 1).  A stored byte is a literal token.  Symbols are decoded with a
// primary table of kInfFastBits bits; a longer code is finished by the canonical walk (first code and count per length).  What zlib
// accepts is accepted and what it refuses is refused: an incomplete code is allowed only where it is a single code of one bit.
#pragma once

#include "dbgk_gz_frame.h"

#ifdef DBGK_INF_COUNT_ITERATIONS   // tests: every iteration of a data-driven loop is counted
#define DBGK_INF_ITER(c) (++(c))
#else
#define DBGK_INF_ITER(c) ((void)0)
#endif

namespace dbgk {
namespace inf {

// the verdict of a member (DBGK_INF_* of include/dbgk.h)
enum Reason : uint32_t {
	R_OK = 0,
	R_BLOCK_TYPE = 1,      // block type 3
	R_STORED_LEN = 2,      // LEN != ~NLEN
	R_STORED_PAST = 3,     // a stored block longer than what is left of the stream
	R_TOO_MANY_SYMS = 4,   // HLIT above 286 or HDIST above 30
	R_CL_OVER = 5,         // the code of the code lengths: over-subscribed
	R_CL_INCOMPLETE = 6,   //   incomplete
	R_CODE_OVER = 7,       // the literal/length or the distance code: over-subscribed
	R_CODE_INCOMPLETE = 8, //   incomplete and not a single code of one bit
	R_REPEAT_FIRST = 9,    // repeat code 16 with no length in front
	R_REPEAT_PAST = 10,    // a repeat that runs past HLIT + HDIST
	R_NO_EOB = 11,         // no code for symbol 256
	R_BAD_LENGTH = 12,     // length symbol 286 or 287, or bits that are no code
	R_BAD_DISTANCE = 13,   // distance symbol 30 or 31, or bits that are no code
	R_DISTANCE_FAR = 14,   // a distance that reaches in front of the member's first byte
	R_TRUNCATED = 15,      // the stream ends inside a block
	R_GARBAGE = 16,        // the final block ends before the trailer
	R_OUT_MORE = 17,       // more output than ISIZE
	R_OUT_LESS = 18,       // less output than ISIZE
	R_CRC = 19,            // the CRC-32 of the output is not the trailer's
	R_FRAME = 20,          // not a member of this framing where the table says one is
	R_COUNT
};

constexpr int kInfFastBits = 9;
constexpr int kInfLitSyms = 288, kInfDistSyms = 32, kInfClSyms = 19, kInfMaxBits = 15;
constexpr int kInfLens = 320; // HLIT + HDIST <= 286 + 30

enum CodeKind { CODE_CL = 0, CODE_LIT = 1, CODE_DIST = 2 };

// the tables of ONE decoder: 2 080 bytes.  Nothing of a decoder is an array on the stack: on the device that would be scratch memory
struct InfTables {
	uint16_t fast[1 << kInfFastBits]; // literal/length code: length << 9 | symbol for the next kInfFastBits bits of the stream; 0: walk
	uint16_t lsym[kInfLitSyms];       // symbols in canonical order
	uint16_t lcnt[kInfMaxBits + 1];   // codes per length
	uint16_t dcnt[kInfMaxBits + 1];
	uint8_t dsym[kInfDistSyms];
	uint8_t lens[kInfLens];           // the lengths as read; the code of the code lengths borrows lsym / lcnt
	uint16_t offs[kInfMaxBits + 1], next[kInfMaxBits + 1]; // inf_build's: first place and next code per length
};

struct InfCount {
	uint32_t n_stored, n_fixed, n_dynamic, n_literals, n_matches;
	uint64_t iterations; // DBGK_INF_COUNT_ITERATIONS only
};

// bits of p[0, n), first bit lowest.  Behind the end the reader gives zeros and sets `over`.
struct InfBits {
	const uint8_t *p;
	uint32_t n, pos, cnt;
	uint64_t buf;
	bool over;
};

DBGK_GZ_HD inline void bits_fill(InfBits &b)
{
	while (b.cnt <= 56u && b.pos < b.n) {
		b.buf |= (uint64_t)b.p[b.pos++] << b.cnt;
		b.cnt += 8u;
	}
}

// the next k <= 16 bits, zeros where the stream has none
DBGK_GZ_HD inline uint32_t bits_peek(InfBits &b, uint32_t k)
{
	if (b.cnt < k) bits_fill(b);
	return (uint32_t)b.buf & ((1u << k) - 1u);
}

DBGK_GZ_HD inline void bits_drop(InfBits &b, uint32_t k)
{
	if (k > b.cnt) {
		b.over = true;
		b.buf = 0;
		b.cnt = 0;
		return;
	}
	b.buf >>= k;
	b.cnt -= k;
}

DBGK_GZ_HD inline uint32_t bits_take(InfBits &b, uint32_t k)
{
	const uint32_t v = bits_peek(b, k);
	bits_drop(b, k);
	return v;
}

DBGK_GZ_HD inline uint32_t bits_used(const InfBits &b) { return 8u * b.pos - b.cnt; }

DBGK_GZ_HD inline uint32_t inf_reverse(uint32_t c, uint32_t len)
{
	uint32_t r = 0;
	for (uint32_t i = 0; i < len; ++i) r |= ((c >> i) & 1u) << (len - 1u - i);
	return r;
}

// lens[0, n) -> cnt[0..15], sym[] in canonical order, and for `fast` != null the primary table.  Returns 0, or 1 over-subscribed,
// 2 incomplete where zlib refuses that: always for the code of the code lengths, else unless the code is one code of one bit.
DBGK_GZ_HD inline int inf_build(const uint8_t *lens, int n, int kind, uint16_t *cnt, uint16_t *sym16, uint8_t *sym8, uint16_t *fast, uint16_t *offs,
                                uint16_t *next)
{
	for (int l = 0; l <= kInfMaxBits; ++l) cnt[l] = 0;
	for (int s = 0; s < n; ++s) cnt[lens[s]]++;
	int left = 1, max = 0;
	for (int l = 1; l <= kInfMaxBits; ++l) {
		left = 2 * left - (int)cnt[l];
		if (left < 0) return 1;
		if (cnt[l]) max = l;
	}
	if (left > 0 && (kind == CODE_CL || max != 1)) {
		if (max != 0 || kind == CODE_CL) return 2; // (no code at all: every symbol is refused where it is met)
	}
	offs[1] = 0;
	next[0] = 0;
	uint32_t c = 0;
	for (int l = 1; l <= kInfMaxBits; ++l) {
		if (l > 1) offs[l] = (uint16_t)(offs[l - 1] + cnt[l - 1]);
		c = (c + (l > 1 ? cnt[l - 1] : 0u)) << 1;
		next[l] = (uint16_t)c;
	}
	if (fast)
		for (int i = 0; i < (1 << kInfFastBits); ++i) fast[i] = 0;
	for (int s = 0; s < n; ++s) {
		const uint32_t l = lens[s];
		if (!l) continue;
		if (sym16) sym16[offs[l]] = (uint16_t)s;
		else sym8[offs[l]] = (uint8_t)s;
		offs[l]++;
		const uint32_t code = next[l]++;
		if (fast && l <= (uint32_t)kInfFastBits)
			for (uint32_t i = inf_reverse(code, l); i < (1u << kInfFastBits); i += 1u << l) fast[i] = (uint16_t)(l << kInfFastBits | (uint32_t)s);
	}
	return 0;
}

// the canonical walk: one bit per iteration.  -1: the bits are no code, or the stream ended
template <typename Sym>
DBGK_GZ_HD inline int inf_walk(InfBits &b, const uint16_t *cnt, const Sym *sym, InfCount &C)
{
	int code = 0, first = 0, index = 0;
	for (int l = 1; l <= kInfMaxBits; ++l) {
		DBGK_INF_ITER(C.iterations);
		code |= (int)bits_take(b, 1);
		if (b.over) return -1;
		const int count = cnt[l];
		if (code - count < first) return (int)sym[index + (code - first)];
		index += count;
		first += count;
		first <<= 1;
		code <<= 1;
	}
	(void)C;
	return -1;
}

DBGK_GZ_HD inline int inf_lit_symbol(InfBits &b, const InfTables &T, InfCount &C)
{
	const uint32_t e = T.fast[bits_peek(b, kInfFastBits)];
	if (e) {
		bits_drop(b, e >> kInfFastBits);
		return b.over ? -1 : (int)(e & ((1u << kInfFastBits) - 1u));
	}
	return inf_walk(b, T.lcnt, T.lsym, C);
}

// length symbol 257..285 -> base and extra bits; distance symbol 0..29 likewise
DBGK_GZ_HD inline void inf_len_base(uint32_t s, uint32_t &base, uint32_t &extra)
{
	const uint32_t i = s - 257u;
	if (i < 8u) { base = 3u + i; extra = 0; return; }
	if (i == 28u) { base = 258u; extra = 0; return; }
	extra = (i - 4u) >> 2;
	base = 3u + ((4u + (i & 3u)) << extra);
}

DBGK_GZ_HD inline void inf_dist_base(uint32_t s, uint32_t &base, uint32_t &extra)
{
	if (s < 4u) { base = 1u + s; extra = 0; return; }
	extra = (s - 2u) >> 1;
	base = 1u + ((2u + (s & 1u)) << extra);
}

// The stream p[0, n) of a member that inflates to `isize` bytes -> *n_tok tokens in tok[0, isize).  Returns the verdict so far: R_OK
// means that the tokens stand for exactly isize bytes and that the final block ends in the stream's last byte; the CRC-32 is the
// resolver's to check.  On another verdict *n_tok is 0.
DBGK_GZ_HD inline uint32_t inf_decode(const uint8_t *p, uint32_t n, uint32_t isize, uint32_t *tok, InfTables &T, uint32_t *n_tok, InfCount &C)
{
	const uint64_t order = 0xF1E2D3C4B5A69780ull; // the places of the code-length code's lengths behind 16, 17, 18: a nibble each
	InfBits b{p, n, 0, 0, 0, false};
	uint32_t nt = 0, out = 0, reason = R_OK;
	*n_tok = 0;
	bool fixed_built = false;
	for (;;) {
		DBGK_INF_ITER(C.iterations);
		const uint32_t last = bits_take(b, 1), type = bits_take(b, 2);
		if (b.over) { reason = R_TRUNCATED; break; }
		if (type == 3u) { reason = R_BLOCK_TYPE; break; }
		if (type == 0u) {
			bits_drop(b, b.cnt & 7u);
			const uint32_t len = bits_take(b, 16), nlen = bits_take(b, 16);
			if (b.over) { reason = R_TRUNCATED; break; }
			if ((len ^ nlen) != 0xFFFFu) { reason = R_STORED_LEN; break; }
			if (len > b.cnt / 8u + (b.n - b.pos)) { reason = R_STORED_PAST; break; }
			if (len > isize - out) { reason = R_OUT_MORE; break; }
			for (uint32_t i = 0; i < len; ++i) {
				DBGK_INF_ITER(C.iterations);
				tok[nt++] = bits_take(b, 8);
			}
			out += len;
			C.n_stored++;
			C.n_literals += len;
		} else {
			// the lengths of both codes in T.lens: hlit literal/length ones, then hdist distance ones
			uint32_t hlit = kInfLitSyms, hdist = kInfDistSyms;
			bool build = true;
			if (type == 1u) {
				build = !fixed_built;
				if (build) {
					for (int s = 0; s < kInfLitSyms; ++s) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
					for (int s = 0; s < kInfDistSyms; ++s) T.lens[kInfLitSyms + s] = 5;
				}
				fixed_built = true;
				C.n_fixed++;
			} else {
				fixed_built = false;
				hlit = bits_take(b, 5) + 257u, hdist = bits_take(b, 5) + 1u;
				const uint32_t hclen = bits_take(b, 4) + 4u;
				if (b.over) { reason = R_TRUNCATED; break; }
				if (hlit > 286u || hdist > 30u) { reason = R_TOO_MANY_SYMS; break; }
				for (int s = 0; s < kInfClSyms; ++s) T.lens[s] = 0;
				for (uint32_t i = 0; i < hclen; ++i) T.lens[i < 3u ? 16u + i : (uint32_t)(order >> (4u * (i - 3u))) & 15u] = (uint8_t)bits_take(b, 3);
				if (b.over) { reason = R_TRUNCATED; break; }
				const int rc = inf_build(T.lens, kInfClSyms, CODE_CL, T.lcnt, T.lsym, nullptr, nullptr, T.offs, T.next);
				if (rc) { reason = rc == 1 ? R_CL_OVER : R_CL_INCOMPLETE; break; }
				uint32_t have = 0;
				while (have < hlit + hdist) {
					DBGK_INF_ITER(C.iterations);
					const int s = inf_walk(b, T.lcnt, T.lsym, C);
					if (s < 0) { reason = b.over ? R_TRUNCATED : R_CL_INCOMPLETE; break; }
					if (s < 16) {
						T.lens[have++] = (uint8_t)s;
						continue;
					}
					uint32_t rep, val = 0;
					if (s == 16) {
						if (!have) { reason = R_REPEAT_FIRST; break; }
						val = T.lens[have - 1u];
						rep = 3u + bits_take(b, 2);
					} else if (s == 17)
						rep = 3u + bits_take(b, 3);
					else
						rep = 11u + bits_take(b, 7);
					if (b.over) { reason = R_TRUNCATED; break; }
					if (have + rep > hlit + hdist) { reason = R_REPEAT_PAST; break; }
					for (uint32_t i = 0; i < rep; ++i) T.lens[have++] = (uint8_t)val;
				}
				if (reason) break;
				if (T.lens[256] == 0) { reason = R_NO_EOB; break; }
				C.n_dynamic++;
			}
			if (build) {
				const int rd = inf_build(T.lens + hlit, (int)hdist, CODE_DIST, T.dcnt, nullptr, T.dsym, nullptr, T.offs, T.next);
				const int rl = inf_build(T.lens, (int)hlit, CODE_LIT, T.lcnt, T.lsym, nullptr, T.fast, T.offs, T.next);
				if (rl || rd) { reason = (rl ? rl : rd) == 1 ? R_CODE_OVER : R_CODE_INCOMPLETE; break; }
			}
			for (;;) {
				DBGK_INF_ITER(C.iterations);
				const int s = inf_lit_symbol(b, T, C);
				if (s < 0) { reason = b.over ? R_TRUNCATED : R_BAD_LENGTH; break; }
				if (s < 256) {
					if (out >= isize) { reason = R_OUT_MORE; break; }
					tok[nt++] = (uint32_t)s;
					out++;
					C.n_literals++;
					continue;
				}
				if (s == 256) break;
				if (s > 285) { reason = R_BAD_LENGTH; break; }
				uint32_t base, extra;
				inf_len_base((uint32_t)s, base, extra);
				const uint32_t len = base + bits_take(b, extra);
				const int d = inf_walk(b, T.dcnt, T.dsym, C);
				if (d < 0) { reason = b.over ? R_TRUNCATED : R_BAD_DISTANCE; break; }
				if (d > 29) { reason = R_BAD_DISTANCE; break; }
				inf_dist_base((uint32_t)d, base, extra);
				const uint32_t dist = base + bits_take(b, extra);
				if (b.over) { reason = R_TRUNCATED; break; }
				if (dist > out) { reason = R_DISTANCE_FAR; break; }
				if (len > isize - out) { reason = R_OUT_MORE; break; }
				tok[nt++] = 0x80000000u | (len - 3u) << 15 | (dist - 1u);
				out += len;
				C.n_matches++;
			}
			if (reason) break;
		}
		if (b.over) { reason = R_TRUNCATED; break; }
		if (last) {
			if ((bits_used(b) + 7u) / 8u != n) reason = R_GARBAGE;
			else if (out != isize) reason = R_OUT_LESS;
			break;
		}
	}
	*n_tok = reason ? 0u : nt;
	return reason;
}

// the frame of one member m[0, size): R_OK and its ISIZE and CRC-32, or R_FRAME
DBGK_GZ_HD inline uint32_t inf_frame(const uint8_t *m, uint64_t size, uint32_t *isize, uint32_t *crc)
{
	*isize = 0;
	*crc = 0;
	if (size < gzf::kGzHead + gzf::kGzTail + 2u || size > gzf::kGzSlot) return R_FRAME;
	uint64_t a = 0, b = 0;
	for (int i = 0; i < 8; ++i) a |= (uint64_t)m[i] << (8 * i), b |= (uint64_t)m[8 + i] << (8 * i);
	if (a != 0x0000000004088b1full || b != 0x000243420006ff00ull) return R_FRAME; // the 16 fixed bytes of dbgk_gz_frame.h
	if (((uint32_t)m[16] | (uint32_t)m[17] << 8) + 1u != (uint32_t)size) return R_FRAME;
	const uint8_t *t = m + size - gzf::kGzTail;
	const uint32_t n = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
	if (n > gzf::kGzPiece) return R_FRAME;
	*crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
	*isize = n;
	return R_OK;
}

} // namespace inf
} // namespace dbgk
