// ANNOT: the annotation bin/correct_error_reads appends to every header (host/correct_error_reads.cpp:172), composed on the device
// from the corrector's records and the compact offsets, so that the formatter (dbgk_format.h) reads its suffix plane where it lies.
// Suffix i, without the final "\n":
//   "\tModifiedBaseNum: " M "\tFinalReadLength: " F "\tLeftEndTrim: " Lt "\tRightEndTrim: " Rt "\tIsDeleted: " D
// M = (uint32)(one_base + tree), F = the record's length in the compact batch (CorrRule::out_len of dbgk_emit.h), Lt / Rt the trims as
// stored, D = deleted as an unsigned number; all in decimal without padding.  Host side: dbgk_host_annot.h.
//
//   k_annot_len      one thread per record: 77 literal bytes + the five digit counts, each nine comparisons with a power of ten
//   (scan)           lengths -> n + 1 suffix offsets, 64 bit (dbgk_sort.hip, rocPRIM)
//   k_annot_write    a workgroup owns kAnnotGroup records in a row, a thread one of them.  The thread composes its suffix in
//                    registers -- the literals are compile-time dwords, a number is eight multiply-shift steps that leave its ASCII
//                    digits in a 64-bit register -- and stores it into LDS at its offset relative to the group's first byte (rounded
//                    down to 16, so LDS and output agree mod 16) with aligned ds_write_b32; only the dword it shares with the record
//                    in front and its last partial dword are byte stores.  The span is then copied out with one ds_read_b128 and one
//                    aligned 16-byte store per lane and round.
//   k_annot_check    what dbgk_fmt_records_device_suffix has to find on the device about a suffix plane of the caller's: offsets
//                    that do not start at 0, that decrease, or whose total reaches 2^32
//
// Which group writes a 16-byte vector that two groups share: the group the vector STARTS in.  It needs up to 15 bytes of the next
// group's first suffix for that -- which are bytes of the first literal whatever the record holds (the literal is longer than 15
// bytes, asserted below) -- or the zero pad behind the last suffix.  So no group reads a record of another one, and no kernel waits
// for another workgroup.
//
// LDS: kAnnotGroup * kAnnotMax + 32 bytes (30 752), five workgroups per CU.  The ds_write_b32 of a wave's 64 records land
// about a suffix apart (~ 90 bytes), which spreads them over the banks but not evenly; what that costs is not profiled.
#pragma once

#include <utility>

#include "dbgk_emit.h"

namespace dbgk {
namespace annotk {

using emitk::kEmitBlock;

// A literal of the annotation: its length, and the dword of its bytes from byte `at` on (bytes behind its end are 0) as a constant
// expression -- the write kernel never indexes a string at run time.
#define DBGK_ANNOT_LITERAL(Name, text)                                                                                                    \
	struct Name {                                                                                                                         \
		static constexpr uint32_t n = sizeof(text) - 1;                                                                                   \
		static constexpr __host__ __device__ uint32_t word(uint32_t at)                                                                   \
		{                                                                                                                                 \
			uint32_t w = 0;                                                                                                               \
			for (uint32_t k = 0; k < 4 && at + k < n; ++k) w |= (uint32_t)(uint8_t)text[at + k] << (8 * k);                               \
			return w;                                                                                                                     \
		}                                                                                                                                 \
	}
DBGK_ANNOT_LITERAL(LitModified, "\tModifiedBaseNum: ");
DBGK_ANNOT_LITERAL(LitFinal, "\tFinalReadLength: ");
DBGK_ANNOT_LITERAL(LitLeft, "\tLeftEndTrim: ");
DBGK_ANNOT_LITERAL(LitRight, "\tRightEndTrim: ");
DBGK_ANNOT_LITERAL(LitDeleted, "\tIsDeleted: ");
#undef DBGK_ANNOT_LITERAL

constexpr uint32_t kAnnotLiteralBytes = LitModified::n + LitFinal::n + LitLeft::n + LitRight::n + LitDeleted::n;
// four 32-bit numbers of at most 10 digits and a byte of at most 3.  (The kernels' own records stay below it: F is 1 digit when the
// trims have 10, and a read is shorter than 2^29 bytes.)
constexpr uint32_t kAnnotMax = kAnnotLiteralBytes + 4 * 10 + 3;
static_assert(kAnnotMax == DBGK_CORR_ANNOT_MAX, "include/dbgk.h states the bound");
static_assert(LitModified::n >= 15, "the bytes a group writes behind its span are bytes of the first literal");

constexpr int kAnnotGroup = kEmitBlock; // records of a workgroup round: one per thread
constexpr uint32_t kAnnotLds = kAnnotGroup * kAnnotMax + 32; // up to 15 bytes in front of the span, its last vector filled up behind

// decimal digits of x: no division, no loop
__device__ __forceinline__ uint32_t digits10(uint32_t x)
{
	return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) + (x >= 100000000u) +
	       (x >= 1000000000u);
}

// the five numbers of record i in the order they are printed
struct Fields {
	uint32_t v[5];
	__device__ __forceinline__ Fields(const dbgk_corr_rec *__restrict__ rec, const uint64_t *__restrict__ coff, uint64_t i)
	{
		const dbgk_corr_rec q = rec[i];
		v[0] = q.one_base + q.tree; // (wraps as the host's %u of the uint32 sum does)
		v[1] = (uint32_t)(coff[i + 1] - coff[i]);
		v[2] = q.left_trim;
		v[3] = q.right_trim;
		v[4] = q.deleted;
	}
	__device__ __forceinline__ uint32_t bytes() const
	{
		return kAnnotLiteralBytes + digits10(v[0]) + digits10(v[1]) + digits10(v[2]) + digits10(v[3]) + digits10(v[4]);
	}
};

// len[i] for i < n, len[n] = 0: the scan runs over n + 1 entries, its last output is the total
__global__ __launch_bounds__(kEmitBlock) void k_annot_len(const dbgk_corr_rec *__restrict__ rec, const uint64_t *__restrict__ coff, uint32_t n,
                                                          uint32_t *__restrict__ len)
{
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i <= n; i += stride) len[i] = i == n ? 0u : Fields(rec, coff, i).bytes();
}

// The bytes of one suffix on their way into LDS: up to 3 of them wait in `w` for the dword they belong to.
struct Composer {
	uint8_t *lds;
	uint32_t at;   // LDS byte of the next dword (a multiple of 4)
	uint32_t nb;   // bytes waiting in w, the first of them its lowest byte
	uint32_t skip; // bytes of the first dword that belong to the record in front: that dword is stored byte by byte
	uint64_t w;

	__device__ __forceinline__ Composer(uint8_t *span, uint32_t start) : lds(span), at(start & ~3u), nb(start & 3u), skip(start & 3u), w(0) {}

	// c bytes (1..4), the first one the lowest byte of v; the bytes of v above them are 0
	__device__ __forceinline__ void put(uint32_t v, uint32_t c)
	{
		w |= (uint64_t)v << (8u * nb);
		nb += c;
		if (nb >= 4u) {
			const uint32_t x = (uint32_t)w;
			if (skip) {
				for (uint32_t k = skip; k < 4u; ++k) lds[at + k] = (uint8_t)(x >> (8u * k));
				skip = 0;
			} else {
				*reinterpret_cast<uint32_t *>(lds + at) = x;
			}
			at += 4u;
			w >>= 32;
			nb -= 4u;
		}
	}

	template <class L, size_t... I>
	__device__ __forceinline__ void literal(std::index_sequence<I...>)
	{
		(put(std::integral_constant<uint32_t, L::word(4 * I)>::value, L::n - 4 * I < 4 ? L::n - 4 * I : 4u), ...);
	}
	template <class L>
	__device__ __forceinline__ void literal()
	{
		literal<L>(std::make_index_sequence<(L::n + 3) / 4>());
	}

	// x < 10^8 -> its eight decimal digits in ASCII, leading zeros included, the first digit in the lowest byte.  x / 10 is one
	// multiply-shift, exact for every 32-bit x.
	static __device__ __forceinline__ uint64_t ascii8(uint32_t x)
	{
		uint64_t p = 0;
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			const uint32_t q = (uint32_t)(((uint64_t)x * 0xCCCCCCCDull) >> 35);
			p = (p << 8) | (uint64_t)('0' + (x - 10u * q));
			x = q;
		}
		return p;
	}

	// x in decimal without padding; d = digits10(x)
	__device__ __forceinline__ void number(uint32_t x, uint32_t d)
	{
		if (d > 8u) { // one or two digits in front of eight
			const uint32_t hi = (uint32_t)(((uint64_t)x * 0xABCC7712ull) >> 58); // x / 10^8, exact for every 32-bit x (checked on the host: tests)
			put((uint32_t)(ascii8(hi) >> (8u * (16u - d))), d - 8u);
			const uint64_t p = ascii8(x - hi * 100000000u);
			put((uint32_t)p, 4u);
			put((uint32_t)(p >> 32), 4u);
		} else {
			const uint64_t p = ascii8(x) >> (8u * (8u - d));
			if (d > 4u) {
				put((uint32_t)p, 4u);
				put((uint32_t)(p >> 32), d - 4u);
			} else {
				put((uint32_t)p, d);
			}
		}
	}

	// the last bytes of the suffix (it is longer than a dword: skip is 0 by now)
	__device__ __forceinline__ void finish()
	{
		for (uint32_t k = 0; k < nb; ++k) lds[at + k] = (uint8_t)(w >> (8u * k));
	}
};

// soff: the n + 1 suffix offsets (soff[0] = 0), n > 0.  dst holds (soff[n] + 15) / 16 16-byte vectors, the pad of the last one is
// written as 0.
__global__ __launch_bounds__(kEmitBlock) void k_annot_write(const dbgk_corr_rec *__restrict__ rec, const uint64_t *__restrict__ coff,
                                                            const uint64_t *__restrict__ soff, uint32_t n, uint4 *__restrict__ dst)
{
	__shared__ __attribute__((aligned(16))) uint8_t span[kAnnotLds];
	const uint32_t tid = threadIdx.x;
	const uint64_t n_groups = ((uint64_t)n + kAnnotGroup - 1) / kAnnotGroup;
	for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
		const uint64_t g0 = g * kAnnotGroup, g1 = g0 + kAnnotGroup < n ? g0 + kAnnotGroup : n;
		const uint64_t base = soff[g0], end = soff[g1];
		const uint64_t lbase = base & ~15ull; // LDS byte 0 is output byte lbase
		const uint64_t i = g0 + tid;
		if (i < g1) {
			const Fields f(rec, coff, i);
			Composer c(span, (uint32_t)(soff[i] - lbase));
			c.literal<LitModified>();
			c.number(f.v[0], digits10(f.v[0]));
			c.literal<LitFinal>();
			c.number(f.v[1], digits10(f.v[1]));
			c.literal<LitLeft>();
			c.number(f.v[2], digits10(f.v[2]));
			c.literal<LitRight>();
			c.number(f.v[3], digits10(f.v[3]));
			c.literal<LitDeleted>();
			c.number(f.v[4], digits10(f.v[4]));
			c.finish();
		}
		// behind the span up to the end of its last vector: the first bytes of the next group's first suffix, or the pad
		const uint32_t e = (uint32_t)(end - lbase), e16 = (e + 15u) & ~15u;
		if (tid < e16 - e) {
			constexpr uint64_t lo = LitModified::word(0) | (uint64_t)LitModified::word(4) << 32, hi = LitModified::word(8) | (uint64_t)LitModified::word(12) << 32;
			const uint32_t b = (uint32_t)((tid < 8u ? lo >> (8u * tid) : hi >> (8u * (tid - 8u))) & 0xFFu);
			span[e + tid] = g1 < n ? (uint8_t)b : (uint8_t)0;
		}
		__syncthreads();
		// the vectors that start inside the span: the one `base` lies in belongs to the group in front unless it starts there
		for (uint32_t v = (base != lbase ? 1u : 0u) + tid; v < e16 / 16u; v += kAnnotGroup) dst[(lbase >> 4) + v] = reinterpret_cast<const uint4 *>(span)[v];
		__syncthreads(); // the span is rewritten by the next round
	}
}

// *bad = 1 if the n + 1 offsets (n > 0) do not start at 0, decrease, or end at 2^32 or behind it; never written otherwise
__global__ __launch_bounds__(kEmitBlock) void k_annot_check(const uint64_t *__restrict__ soff, uint32_t n, uint32_t *__restrict__ bad)
{
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i < n; i += stride) {
		const uint64_t a = soff[i], b = soff[i + 1];
		if ((i == 0 && a != 0) || b < a || (i + 1 == n && (b >> 32))) *bad = 1u;
	}
}

} // namespace annotk
} // namespace dbgk
