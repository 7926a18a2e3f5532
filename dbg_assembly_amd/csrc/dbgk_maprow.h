// ROWS: the lines bin/map_reads and bin/map_pair write for a batch of hits (host/map_reads.cpp, host/map_pair.cpp, Contigs::row of
// host/map_common.h), composed on the device from the parser's batch, the mapper's hits and the caller's contig table.  An ITEM is a
// read (READS: hits 2 i and 2 i + 1 are its two alignments) or a pair (PAIR: read i of side 0 and read i of side 1, the first hit of
// each).  A ROW SLOT is alignment j (0 / 1) of item i; both modes reach it the same way -- side j, read i, hit 2 i of that side --
// because the host hands READS a side 1 that is side 0 with its hits moved on by one.  Host side: dbgk_host_maprow.h.
//
//   k_maprow_ids     one thread per read of a side: the spans of the first two tokens of its header under the delimiter set
//   k_maprow_len     one thread per item: its class, its byte length in each of the three streams (digit counts by comparisons, the
//                    identity's length from the rule of dbgk_maprow_rule.h), what makes a batch unusable (a contig outside the table,
//                    a negative coordinate, mismatches outside [0, align_len], offsets that decrease, a header outside the text), and
//                    the counters, folded per wave and workgroup as fold_counters does
//   (scan)           per stream, lengths -> n + 1 output offsets, 64 bit (dbgk_sort.hip, rocPRIM)
//   k_maprow_num     one thread per row slot that is printed: the two numeric segments of the row
//                      A  "\t" read_len "\t" read_start "\t" read_end "\t"                                             (<= 34 bytes)
//                      B  "\t" contig_len "\t" contig_start "\t" contig_end "\t" direct "\t" identity "%" ("\t" | "\n")  (<= 49 bytes)
//                    composed into the thread's 112 bytes of LDS by annotk::Composer and copied to the slot's 112 bytes of the
//                    segment plane in 16-byte stores: A at byte 0, the two lengths as one dword at byte 44, B at byte 48
//   k_maprow_write   tiled by OUTPUT as k_fmt_gather is: a workgroup owns kEmitTile bytes of a stream, a lane one aligned 16-byte vector.
//                    The lane finds its item by bisection in the stream's offsets, the row inside the item's line from the first
//                    row's length, and inside the row the piece that holds an output byte -- token, "-", token, A, contig id, B; for
//                    the FASTA stream ">", token, "-", token, "\n", bases, "\n" -- from six cumulative lengths.  An output dword inside
//                    one source piece is composed from the aligned source dwords that hold its bytes, every other dword byte by
//                    byte.  One aligned 16-byte store per lane; the pad behind the stream is 0.  Two forms: rows, FASTA.
// No kernel waits for another workgroup: every hand-over is the end of a launch.  No byte goes to global memory on its own.
//
// Known costs, none profiled apart: the segment plane is sized for every slot (224 bytes per item) though only printed slots are
// written and read; a lane that enters a row reloads that row's numbers with dependent loads (token spans, the length dword, the
// hit's contig, two name offsets), once per row and lane -- a row is 60 to 120 bytes, so about every sixth lane does; the bytes of
// thread t's LDS slot start 28 t dwords in, which maps 16 threads of a wave to four banks' worth of distinct starts.
#pragma once

#include "dbgk_annot.h"
#include "dbgk_emit.h"
#include "dbgk_maprow_rule.h"
#include "dbgk_pair.h"

namespace dbgk {
namespace rowk {

using emitk::kEmitBlock;
using emitk::kEmitTile;
using emitk::kWave;
static_assert(DBGK_MAPROW_TILE == kEmitTile, "one 16-byte store per lane writes a tile");

constexpr uint32_t kSlot = 112, kSegB = 48, kLenAt = 44; // a row slot of the segment plane
constexpr uint32_t kSegAMax = 4 + 3 * 10, kSegBMax = 8 + 3 * 10 + maprule::kIdentMax;
static_assert(kSegAMax <= kLenAt && kSegB + kSegBMax <= kSlot && kSlot % 16 == 0 && kLenAt % 4 == 0 && kSegB % 4 == 0, "the slot holds both segments");

enum Counter { RC_TOTAL = 0, RC_C1, RC_C2, RC_C3, RC_C4, RC_UNPRINTABLE, RC_BAD, RC_COUNT };
// what an item writes: nothing; both rows as one line of stream 0; READS row 0 / PAIR both rows in stream 1; PAIR row 0 or row 1 alone in
// stream 2.  CL_LINE0 of READS also writes the read to stream 2.
enum Class : uint32_t { CL_NONE = 0, CL_LINE0, CL_LINE1, CL_GAP0, CL_GAP1 };

struct RowSide {
	const uint8_t *text;
	const dbgk_parse_rec *recs;
	const uint8_t *bases;
	const uint64_t *off;
	const dbgk_map_hit *hits; // slot j of item i: hits[2 i] of side j
	const uint4 *ids;         // per read: position and length of the first token, of the second one (length 0: there is none)
};

struct RowIn {
	RowSide s[2];
	const uint8_t *names;
	const uint64_t *name_off;
	const uint32_t *ctg_len;
	uint32_t n_contigs;
	uint32_t pair;    // 1: PAIR, 0: READS
	uint32_t min_len;
};

__device__ __forceinline__ RowSide side_of(const RowIn &in, uint32_t j) { return j ? in.s[1] : in.s[0]; }

__device__ __forceinline__ bool is_delim(uint32_t c, uint64_t dlo, uint64_t dhi)
{
	const uint64_t m = c < 64u ? dlo : dhi;
	return c < 128u && ((m >> (c & 63u)) & 1u);
}

// what k_maprow_ids reads and writes (a struct, so that no record type of another stage becomes part of the kernel's name)
struct IdsIn {
	const uint8_t *text;
	const dbgk_parse_rec *recs;
	uint4 *ids;
	uint32_t *bad;
};

// ids[i] for the n reads of one side.  A header that leaves the text sets *bad and gets empty tokens.
__global__ __launch_bounds__(kEmitBlock) void k_maprow_ids(IdsIn in, uint32_t n, uint32_t n_text, uint64_t dlo, uint64_t dhi)
{
	const uint8_t *__restrict__ text = in.text;
	const dbgk_parse_rec *__restrict__ recs = in.recs;
	uint4 *__restrict__ ids = in.ids;
	uint32_t *__restrict__ bad = in.bad;
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i < n; i += stride) {
		const uint32_t hp = recs[i].head_pos, hl = recs[i].head_len;
		if ((uint64_t)hp + hl > n_text) {
			*bad = 1u;
			ids[i] = uint4{0, 0, 0, 0};
			continue;
		}
		uint32_t p = hp;
		const uint32_t end = hp + hl;
		while (p < end && is_delim(text[p], dlo, dhi)) ++p;
		const uint32_t t0 = p;
		while (p < end && !is_delim(text[p], dlo, dhi)) ++p;
		const uint32_t l0 = p - t0;
		while (p < end && is_delim(text[p], dlo, dhi)) ++p;
		const uint32_t t1 = p;
		while (p < end && !is_delim(text[p], dlo, dhi)) ++p;
		ids[i] = uint4{t0, l0, t1, p - t1};
	}
}

// the identity field of a hit with 0 <= mismatches <= align_len, align_len > 0
__device__ __forceinline__ maprule::IdentText ident_of(const dbgk_map_hit &h)
{
	return maprule::ident_text(maprule::ident_value(__fdiv_rn((float)h.mismatches, (float)h.align_len)));
}

__device__ __forceinline__ uint32_t id_bytes(const uint4 &t) { return t.y + (t.w ? 1u + t.w : 0u); }

// The bytes of row slot (i, side S) with its terminator; rl: the read's length.  A hit no row can be made of sets `bad`, an
// identity %g would print in exponent form `unprintable`.
__device__ __forceinline__ uint64_t row_bytes(const RowIn &in, const RowSide &S, uint64_t i, uint32_t rl, uint32_t &bad, uint32_t &unprintable)
{
	const dbgk_map_hit h = S.hits[2 * i];
	if (h.contig < 0 || (uint32_t)h.contig >= in.n_contigs || h.read_start < 0 || h.read_end < 0 || h.contig_start < 0 || h.contig_end < 0 || h.align_len <= 0 ||
	    h.mismatches < 0 || h.mismatches > h.align_len) {
		bad++;
		return 0;
	}
	const uint32_t nt = ident_of(h).n;
	if (!nt) unprintable++;
	const uint64_t name = in.name_off[h.contig + 1] - in.name_off[h.contig];
	return (uint64_t)id_bytes(S.ids[i]) + 4u + annotk::digits10(rl) + annotk::digits10((uint32_t)h.read_start) + annotk::digits10((uint32_t)h.read_end) + name + 8u +
	       annotk::digits10(in.ctg_len[h.contig]) + annotk::digits10((uint32_t)h.contig_start) + annotk::digits10((uint32_t)h.contig_end) + nt;
}

// whether row slot j of an item of class c is printed
__device__ __forceinline__ bool slot_printed(uint32_t pair, uint32_t c, uint32_t j)
{
	if (c == CL_LINE0) return true;
	if (c == CL_LINE1) return pair || j == 0u;
	return (c == CL_GAP0 && j == 0u) || (c == CL_GAP1 && j == 1u);
}

// len0 / len1 / len2[i] and cls[i] for i < n; len*[n] = 0: the scans run over n + 1 entries, their last output is the total.
__global__ __launch_bounds__(kEmitBlock) void k_maprow_len(RowIn in, uint32_t n, uint32_t *__restrict__ len0, uint32_t *__restrict__ len1,
                                                           uint32_t *__restrict__ len2, uint32_t *__restrict__ cls, unsigned long long *__restrict__ counters)
{
	unsigned long long total = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
	uint32_t bad = 0, unprintable = 0;
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
#pragma unroll 1
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i <= n; i += stride) {
		uint64_t l0 = 0, l1 = 0, l2 = 0;
		if (i < n) {
			uint32_t c = CL_NONE;
			const uint64_t oa = in.s[0].off[i], ob = in.s[0].off[i + 1];
			uint64_t La = ob - oa, Lb = La;
			bool ok = ob >= oa && !(La >> 31);
			if (in.pair) {
				const uint64_t pa = in.s[1].off[i], pb = in.s[1].off[i + 1];
				Lb = pb - pa;
				ok = ok && pb >= pa && !(Lb >> 31);
			}
			if (!ok) {
				bad++;
			} else if (La >= in.min_len && Lb >= in.min_len) {
				const bool ma = in.s[0].hits[2 * i].contig != -1, mb = in.s[1].hits[2 * i].contig != -1;
				const bool diff = in.s[0].hits[2 * i].contig != in.s[1].hits[2 * i].contig;
				total++;
				if (!in.pair) {
					// map_reads.cpp: a and b on two contigs -> a 2ctg line and the read; a alone -> a 1ctg line; both on one contig -> counted only
					if (ma && mb) {
						if (diff) c1++, c = CL_LINE0;
						else c4++;
					} else if (ma) {
						c2++, c = CL_LINE1;
					} else {
						c3++;
					}
				} else {
					// map_pair.cpp: both mates mapped -> one line, 2ctg or 1ctg; one mate -> its row in the gap file
					if (ma && mb) {
						if (diff) c1++, c = CL_LINE0;
						else c2++, c = CL_LINE1;
					} else if (ma || mb) {
						c3++, c = ma ? CL_GAP0 : CL_GAP1;
					} else {
						c4++;
					}
				}
			}
			uint64_t m = 0; // the rows of the item's line
#pragma unroll 1
			for (uint32_t j = 0; j < 2u; ++j)
				if (slot_printed(in.pair, c, j)) m += row_bytes(in, side_of(in, j), i, (uint32_t)(j ? Lb : La), bad, unprintable);
			if (c == CL_LINE0) {
				l0 = m;
				if (!in.pair) l2 = (uint64_t)id_bytes(in.s[0].ids[i]) + La + 3u;
			} else if (c == CL_LINE1) {
				l1 = m;
			} else {
				l2 = m;
			}
			if ((l0 >> 32) || (l1 >> 32) || (l2 >> 32)) {
				bad++;
				l0 = l1 = l2 = 0;
			}
			cls[i] = c;
		}
		len0[i] = (uint32_t)l0;
		len1[i] = (uint32_t)l1;
		len2[i] = (uint32_t)l2;
	}
	const unsigned long long v[RC_COUNT] = {total, c1, c2, c3, c4, unprintable, bad};
	emitk::fold_counters(v, counters);
}

// plane: 2 n slots of kSlot bytes.  A workgroup round composes kEmitBlock slots in LDS and copies the printed ones out.  The batch has
// passed k_maprow_len without a bad or unprintable hit.
__global__ __launch_bounds__(kEmitBlock) void k_maprow_num(RowIn in, const uint32_t *__restrict__ cls, uint32_t n, uint4 *__restrict__ plane)
{
	__shared__ __attribute__((aligned(16))) uint8_t lds[kEmitBlock * kSlot];
	const uint32_t tid = threadIdx.x;
	const uint64_t n_slots = 2ull * n, n_groups = (n_slots + kEmitBlock - 1) / kEmitBlock;
	for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
		const uint64_t slot = g * kEmitBlock + tid;
		uint32_t words = 0;
		if (slot < n_slots) {
			const uint64_t i = slot >> 1;
			const uint32_t j = (uint32_t)slot & 1u, c = cls[i];
			if (slot_printed(in.pair, c, j)) {
				const RowSide S = side_of(in, j);
				const dbgk_map_hit h = S.hits[2 * i];
				const uint32_t rl = (uint32_t)(S.off[i + 1] - S.off[i]), cl = in.ctg_len[h.contig];
				// the first row of a line of two ends in a tab, every other row ends its line
				const bool first_of_two = j == 0u && (c == CL_LINE0 || (c == CL_LINE1 && in.pair));
#pragma unroll 1
				for (uint32_t seg = 0; seg < 2u; ++seg) { // A, then B: "\t" number, three times, and the segment's tail
					const uint32_t start = tid * kSlot + seg * kSegB;
					annotk::Composer o(lds, start);
#pragma unroll 1
					for (uint32_t f = 0; f < 3u; ++f) {
						const uint32_t x = seg ? (f == 0u ? cl : f == 1u ? (uint32_t)h.contig_start : (uint32_t)h.contig_end)
						                       : (f == 0u ? rl : f == 1u ? (uint32_t)h.read_start : (uint32_t)h.read_end);
						o.put('\t', 1u);
						o.number(x, annotk::digits10(x));
					}
					if (seg) {
						o.put('\t' | ((uint32_t)h.direct & 0xFFu) << 8 | (uint32_t)'\t' << 16, 3u);
						const maprule::IdentText t = ident_of(h);
						o.put((uint32_t)t.lo, t.n < 4u ? t.n : 4u);
						if (t.n > 4u) o.put((uint32_t)(t.lo >> 32), t.n < 8u ? t.n - 4u : 4u);
						if (t.n > 8u) o.put((uint32_t)t.hi, t.n - 8u);
						o.put('%' | (first_of_two ? (uint32_t)'\t' : (uint32_t)'\n') << 8, 2u);
					} else {
						o.put('\t', 1u);
					}
					o.finish();
					words |= (o.at + o.nb - start) << (8u * seg);
				}
			}
		}
		*reinterpret_cast<uint32_t *>(lds + tid * kSlot + kLenAt) = words; // 0: the slot is not printed and not copied
		__syncthreads();
		constexpr uint32_t kVecs = kSlot / 16;
		for (uint32_t v = tid; v < kEmitBlock * kVecs; v += kEmitBlock) {
			const uint32_t s = v / kVecs;
			if (g * kEmitBlock + s < n_slots && *reinterpret_cast<const uint32_t *>(lds + s * kSlot + kLenAt))
				plane[g * kEmitBlock * kVecs + v] = reinterpret_cast<const uint4 *>(lds)[v];
		}
		__syncthreads(); // the slots are rewritten by the next round
	}
}

// One row, or one FASTA record, as the write kernel sees it: output byte q of the stream is byte q - c0 of it, and b0 .. b6 are the
// ends of its pieces relative to c0.
//   row    (empty)  token  "-"  token  A     contig id  B
//   FASTA  ">"      token  "-"  token  "\n"  bases      "\n"
template <bool FA>
struct RowRec {
	uint64_t c0, e;
	uint64_t a1, a3, a4, a5; // first bytes of token 1, token 2, A (B lies kSegB behind it), the contig id or the bases
	uint32_t b0, b1, b2, b3, b4, b5, b6;

	__device__ __forceinline__ void load(const RowIn &in, const uint8_t *__restrict__ plane, uint64_t i, uint32_t j, uint64_t at)
	{
		const RowSide S = side_of(in, j);
		const uint4 t = S.ids[i];
		c0 = at;
		a1 = (uint64_t)S.text + t.x;
		a3 = (uint64_t)S.text + t.z;
		b0 = FA ? 1u : 0u;
		b1 = b0 + t.y;
		b2 = b1 + (t.w ? 1u : 0u);
		b3 = b2 + t.w;
		if (FA) {
			const uint64_t o = S.off[i];
			a4 = 0;
			a5 = (uint64_t)S.bases + o;
			b4 = b3 + 1u;
			b5 = b4 + (uint32_t)(S.off[i + 1] - o);
			b6 = b5 + 1u;
		} else {
			a4 = (uint64_t)plane + (2 * i + j) * kSlot;
			const uint32_t w = *reinterpret_cast<const uint32_t *>(a4 + kLenAt);
			const int32_t c = S.hits[2 * i].contig;
			const uint64_t no = in.name_off[c];
			a5 = (uint64_t)in.names + no;
			b4 = b3 + (w & 0xFFu);
			b5 = b4 + (uint32_t)(in.name_off[c + 1] - no);
			b6 = b5 + ((w >> 8) & 0xFFu);
		}
		e = c0 + b6;
	}

	// The piece that holds byte `rel` < b6: true and the address of that byte with the piece's end in `lim` for a source piece, false
	// and the byte itself in `sep` for a separator.
	__device__ __forceinline__ bool piece(uint32_t rel, uint64_t &addr, uint32_t &lim, uint32_t &sep) const
	{
		if (rel < b0) {
			sep = '>';
			return false;
		}
		if (rel < b1) {
			addr = a1 + (rel - b0);
			lim = b1;
			return true;
		}
		if (rel < b2) {
			sep = '-';
			return false;
		}
		if (rel < b3) {
			addr = a3 + (rel - b2);
			lim = b3;
			return true;
		}
		if (rel < b4) {
			if (FA) {
				sep = '\n';
				return false;
			}
			addr = a4 + (rel - b3);
			lim = b4;
			return true;
		}
		if (rel < b5) {
			addr = a5 + (rel - b4);
			lim = b5;
			return true;
		}
		if (FA) {
			sep = '\n';
			return false;
		}
		addr = a4 + kSegB + (rel - b5);
		lim = b6;
		return true;
	}
};

// coff: the n + 1 offsets of one stream, total = coff[n] > 0.  two: an item's line holds both of its rows (else the one its class
// names).  dst holds (total + 15) / 16 16-byte vectors, the pad of the last one is written as 0.
template <bool FA>
__global__ __launch_bounds__(kEmitBlock) void k_maprow_write(RowIn in, const uint32_t *__restrict__ cls, const uint8_t *__restrict__ plane,
                                                             const uint64_t *__restrict__ coff, uint32_t n, uint64_t total, uint32_t two,
                                                             uint4 *__restrict__ dst)
{
	__shared__ uint64_t range[2];
	const int tid = (int)threadIdx.x, lane = emitk::lane_id(), wave = tid / kWave;
	const uint64_t n_tiles = (total + kEmitTile - 1) / kEmitTile;
	for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const uint64_t lo = t * kEmitTile, hi = lo + kEmitTile < total ? lo + kEmitTile : total;
		// items [r0, r1) intersect [lo, hi): r0 = the first item that ends behind lo, r1 = the first that starts at or behind hi
		if (wave == 0) {
			const uint64_t r = emitk::wave_search<true>(coff, 1, n, lo, lane);
			if (lane == 0) range[0] = r;
		} else if (wave == 1) {
			const uint64_t r = emitk::wave_search<false>(coff, 0, (uint64_t)n + 1, hi, lane);
			if (lane == 0) range[1] = r;
		}
		__syncthreads();
		const uint64_t r0 = range[0], r1 = range[1] < n ? range[1] : n;
		const uint64_t pos = lo + 16ull * tid;
		if (pos < hi) {
			uint64_t r = emitk::owner_of(coff, r0, r1, pos); // (the last item that starts at or in front of pos: the one that holds it)
			RowRec<FA> R;
			uint32_t k = 0; // the row of the line R is
			R.load(in, plane, r, FA ? 0u : (cls[r] == CL_GAP1 ? 1u : 0u), coff[r]);
			if (!FA && two && pos >= R.e) {
				R.load(in, plane, r, 1u, R.e);
				k = 1;
			}
			uint32_t v[4];
#pragma unroll
			for (int d = 0; d < 4; ++d) {
				const uint64_t p = pos + 4u * d;
				uint32_t x = 0;
				uint64_t addr = 0;
				uint32_t lim = 0, sep = 0;
				bool whole = false; // the dword lies inside one source piece of the current row
				if (p + 4 <= R.e && p < hi) { // (p >= R.c0: R holds the byte in front of p, or p itself)
					const uint32_t rel = (uint32_t)(p - R.c0);
					whole = R.piece(rel, addr, lim, sep) && rel + 4 <= lim;
					if (whole) x = pairk::load_unaligned_at(addr);
				}
				if (!whole) {
#pragma unroll
					for (int b = 0; b < 4; ++b) {
						const uint64_t q = p + b;
						if (q >= hi) break; // behind the stream: the pad stays 0 (a tile ends on a dword unless the stream ends in it)
						if (q >= R.e) {     // no row is empty: the next one holds the byte
							if (!FA && two && k == 0u) {
								R.load(in, plane, r, 1u, R.e);
								k = 1;
							} else {
								r = emitk::owner_of(coff, r + 1, r1, q);
								R.load(in, plane, r, FA ? 0u : (cls[r] == CL_GAP1 ? 1u : 0u), coff[r]);
								k = 0;
							}
						}
						const uint32_t rel = (uint32_t)(q - R.c0);
						const uint32_t byte = R.piece(rel, addr, lim, sep) ? (uint32_t)*reinterpret_cast<const uint8_t *>(addr) : sep;
						x |= byte << (8 * b);
					}
				}
				v[d] = x;
			}
			dst[pos >> 4] = uint4{v[0], v[1], v[2], v[3]};
		}
		__syncthreads(); // the range is rewritten by the next round
	}
}

} // namespace rowk
} // namespace dbgk
