// ROWS: the identity field of a row (host/map_common.h, Contigs::row) as one function for host and device, free of HIP so that a
// plain C++ program can compare it with the stream it restates.  The host prints
//   float identity = 1.0 - (float)mismatches / align_len;   o << identity * 100
// which is three IEEE operations -- a float division, a double subtraction rounded to float, a float multiplication -- and then
// `%g` with precision 6.  Everything behind the three operations is integer work here:
//   v == 0 prints "0".  Otherwise v = M * 2^E with M the 24-bit significand (E < 0: v <= 100 < 2^7).  For X = 2, 1, .., -4 take
//   q = floor(M * 10^(5 - X) * 2^E) in 64 bits (M * 10^9 < 2^54); the first X with q >= 10^5 is the decimal exponent -- of the
//   truncated value, as %g takes it: 0.99999905 prints 0.999999, not 1.  q is rounded half to even on the bits shifted out; a carry
//   to 10^6 gives 10^5 and X + 1.  The six digits are printed with the point behind digit X + 1 (for X < 0: "0.", -X - 1 zeros, the
//   digits), trailing zeros stripped, then a bare point.
// No X fits when 0 < v < 10^-4, where %g turns to its exponent form: such a value is UNPRINTABLE here (n == 0), and so is anything
// the three operations make of mismatches > align_len or align_len == 0 (negative, infinite, NaN).  The text has at most
// kIdentMax = 11 bytes ("0.000123456"), returned packed: byte i of the text is byte i of lo (i < 8) or byte i - 8 of hi.
#pragma once

#include <cstdint>
#include <cstring>

#ifndef DBGK_HD
#define DBGK_HD
#endif

namespace dbgk {
namespace maprule {

constexpr uint32_t kIdentMax = 11;

struct IdentText {
	uint64_t lo, hi;
	uint32_t n; // bytes of the text; 0: unprintable
};

// the value the host streams out; `quot` is the correctly rounded (float)mismatches / (float)align_len, which the caller computes
// (the device with __fdiv_rn: its default division is not the IEEE one)
DBGK_HD inline float ident_value(float quot)
{
	const float identity = (float)(1.0 - (double)quot);
	return identity * 100.0f; // (a float product of a value rounded to float: there is nothing to contract it with)
}

DBGK_HD inline uint32_t ident_pow10(uint32_t e) // e <= 9
{
	uint32_t p = 1;
	for (uint32_t k = 0; k < e; ++k) p *= 10u;
	return p;
}

struct IdentOut {
	IdentText t{0, 0, 0};
	DBGK_HD void put(uint32_t c)
	{
		if (t.n < 8u) t.lo |= (uint64_t)c << (8u * t.n);
		else t.hi |= (uint64_t)c << (8u * (t.n - 8u));
		t.n++;
	}
	// x < 10^width in `width` digits, leading zeros included
	DBGK_HD void digits(uint32_t x, uint32_t width)
	{
		for (uint32_t p = ident_pow10(width ? width - 1u : 0u); width; --width, p /= 10u) {
			const uint32_t d = x / p;
			put('0' + d);
			x -= d * p;
		}
	}
};

DBGK_HD inline IdentText ident_text(float v)
{
	uint32_t bits;
	memcpy(&bits, &v, 4);
	IdentOut o;
	if ((bits << 1) == 0u) { // +0 and -0: the stream prints "0" and "-0"; -0 does not arise (1.0 - q with q <= 1 is +0 at q == 1)
		if (bits == 0u) o.put('0');
		return o.t;
	}
	const uint32_t ex = (bits >> 23) & 0xFFu;
	if ((bits >> 31) || ex == 0xFFu || ex == 0u) return o.t; // negative, infinite, NaN, subnormal
	const uint64_t M = (bits & 0x7FFFFFu) | 0x800000u;
	const int32_t E = (int32_t)ex - 150;
	if (E > -17 || E < -63) return o.t; // v >= 128 (never: v <= 100), or v < 2^-40
	const uint32_t s = (uint32_t)-E;
	int32_t X = 2;
	uint64_t q = 0, P = 0;
	for (; X >= -4; --X) {
		P = M * (uint64_t)ident_pow10((uint32_t)(5 - X));
		q = P >> s;
		if (q >= 100000u) break;
	}
	if (X < -4) return o.t; // 0 < v < 10^-4: %g's exponent form
	const uint64_t rem = P & ((1ull << s) - 1ull), half = 1ull << (s - 1u);
	if (rem > half || (rem == half && (q & 1u))) q++;
	if (q == 1000000u) {
		q = 100000u;
		X++;
	}
	if (X > 2) return o.t; // (never: v <= 100 is 100000 exactly at X = 2)
	uint32_t d = (uint32_t)q, tz = 0;
	while (tz < 5u && d % 10u == 0u) {
		d /= 10u;
		tz++;
	}
	const uint32_t nd = 6u - tz; // d holds the nd significant digits
	if (X >= 0) {
		const uint32_t ni = (uint32_t)X + 1u; // digits in front of the point
		if (nd <= ni) {
			o.digits(d * ident_pow10(ni - nd), ni);
		} else {
			const uint32_t pf = ident_pow10(nd - ni);
			o.digits(d / pf, ni);
			o.put('.');
			o.digits(d % pf, nd - ni);
		}
	} else {
		o.put('0');
		o.put('.');
		for (int32_t k = 0; k < -X - 1; ++k) o.put('0');
		o.digits(d, nd);
	}
	return o.t;
}

} // namespace maprule
} // namespace dbgk
