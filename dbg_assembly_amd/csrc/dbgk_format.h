// FORMAT stage: a compact batch of n records (a bases plane, a quality plane for FASTQ, n + 1 offsets -- the layout dbgk_emit.h
// writes), the header lines where they lie in the text the parser parsed, and an optional suffix plane from the host become the
// text of an output file, record after record:
//   FASTQ  H S "\n" B "\n+\n" Q "\n"        FASTA  H S "\n" B "\n"
// H: the header's bytes (its first byte replaced by `marker` if that is not 0), S: the suffix, B / Q: the record's bytes of the two
// planes.  An emptied record is written with its empty lines; no record is dropped, so no record has length 0.  Host side:
// dbgk_host_format.h.
//
//   k_fmt_len        one thread per record: its output length, the validation (a header that leaves the text, offsets that
//                    decrease, a record of 2^32 bytes and more), and the byte counters -- header, suffix, sequence -- reduced per
//                    wave and workgroup as fold_counters does.
//   (scan)           lengths -> n + 1 output offsets, 64 bit (dbgk_sort.hip, rocPRIM)
//   k_fmt_gather     tiled by OUTPUT as k_emit_gather is: a workgroup owns kEmitTile bytes of text, a lane one 16-byte vector of them.
//                    The tile's records come from the two 64-way searches in the output offsets, a lane's first record by
//                    bisection.  Inside a record the piece that holds an output byte -- header, suffix, "\n", bases, "\n+\n",
//                    quality, "\n" -- follows from six cumulative lengths (three for FASTA) kept relative to the record's start.  An
//                    output dword that lies inside ONE source piece is composed in registers from the aligned source dwords
//                    that hold its bytes; every other dword (a separator in it, a piece or record boundary, the end of the
//                    text) is put together byte by byte, the separators from constants.  One aligned 16-byte store per lane.
//                    Two forms: FASTQ, FASTA.
// No kernel waits for another workgroup: every hand-over is the end of a launch.
//
// Memory the gather reads: a source byte only inside the aligned dwords that hold a byte of the piece being copied -- the second
// dword of a pair is loaded only when it holds one, the byte path loads single bytes.  The text and the planes are 16-byte aligned
// (checked by the host), so no read reaches n_text rounded up to 16, or offsets[n] of a plane rounded up to 4.
//
// Known costs, none profiled apart: the three of the emit gather (dbgk_emit.h) -- here a record of 150 bases has seven pieces, so
// about one dword in 13 takes the byte path; a lane that changes record reloads that record's six numbers (header position and
// length, two plane offsets, two suffix offsets) with dependent loads, which a tile of many tiny records pays once per record and
// lane; the suffix offsets are uploaded as 64-bit numbers where 32 would do.
#pragma once

#include "dbgk_emit.h"
#include "dbgk_pair.h"

namespace dbgk {
namespace fmtk {

using emitk::kEmitBlock;
using emitk::kEmitTile;
using emitk::kWave;
static_assert(DBGK_FMT_TILE == kEmitTile, "one 16-byte store per lane writes a tile");

enum Counter { FC_HEAD = 0, FC_SUFFIX, FC_SEQ, FC_BAD, FC_COUNT };

// what every kernel of the stage reads; quals is read by the FASTQ forms only, suf / soff may both be null (all suffixes empty)
struct FmtIn {
	const uint8_t *text;
	const dbgk_parse_rec *recs;
	const uint8_t *bases, *quals;
	const uint64_t *off;
	const uint8_t *suf;
	const uint64_t *soff;
};

// len[i] for i < n, len[n] = 0: the scan runs over n + 1 entries, its last output is the total.  A record that fails the
// validation gets length 0 and is counted; the host then refuses the batch before any gather.
__global__ __launch_bounds__(kEmitBlock) void k_fmt_len(FmtIn in, uint32_t n, uint32_t n_text, uint32_t fastq, uint32_t *__restrict__ len,
                                                        unsigned long long *__restrict__ counters)
{
	unsigned long long head = 0, suffix = 0, seq = 0;
	uint32_t bad = 0;
	const uint64_t stride = (uint64_t)gridDim.x * kEmitBlock;
#pragma unroll 1
	for (uint64_t i = (uint64_t)blockIdx.x * kEmitBlock + threadIdx.x; i <= n; i += stride) {
		if (i == n) {
			len[i] = 0;
			break;
		}
		const uint64_t hp = in.recs[i].head_pos, hl = in.recs[i].head_len;
		const uint64_t o = in.off[i], o1 = in.off[i + 1];
		const uint64_t sl = in.soff ? in.soff[i + 1] - in.soff[i] : 0; // (checked by the host: they do not decrease)
		const uint64_t L = o1 - o;
		const uint64_t m = fastq ? hl + sl + 2 * L + 5 : hl + sl + L + 2;
		if (o1 < o || hp + hl > n_text || (L >> 32) || (m >> 32)) {
			bad++;
			len[i] = 0;
			continue;
		}
		len[i] = (uint32_t)m;
		head += hl;
		suffix += sl;
		seq += L;
	}
	const unsigned long long v[FC_COUNT] = {head, suffix, seq, bad};
	emitk::fold_counters(v, counters);
}

// One record as the gather sees it: output byte q of the text is byte q - c0 of the record, and b1 .. b6 are the ends of its
// pieces relative to c0 -- header, suffix, "\n", bases, and for FASTQ "\n+\n", quality; the last "\n" ends the record at e.
template <bool FASTQ>
struct FmtRec {
	uint64_t c0, e;
	uint64_t a_head, a_suf, a_seq; // addresses of the first byte of the three sources (the quality's: a_seq - bases + quals)
	uint32_t b1, b2, b4;           // b3 = b2 + 1, b5 = b4 + 3, b6 = b5 + (b4 - b3)

	__device__ __forceinline__ void load(const FmtIn &in, const uint64_t *__restrict__ coff, uint64_t r)
	{
		c0 = coff[r];
		e = coff[r + 1];
		const uint32_t hp = in.recs[r].head_pos, hl = in.recs[r].head_len;
		const uint64_t o = in.off[r];
		const uint32_t L = (uint32_t)(in.off[r + 1] - o);
		uint64_t so = 0;
		uint32_t sl = 0;
		if (in.soff) {
			so = in.soff[r];
			sl = (uint32_t)(in.soff[r + 1] - so);
		}
		a_head = (uint64_t)in.text + hp;
		a_suf = (uint64_t)in.suf + so;
		a_seq = (uint64_t)in.bases + o;
		b1 = hl;
		b2 = hl + sl;
		b4 = b2 + 1 + L;
	}

	// The piece that holds byte `rel` of the record: true and the address of that byte with the piece's end in `lim` for a source
	// piece, false and the byte itself in `sep` for a separator.
	__device__ __forceinline__ bool piece(const FmtIn &in, uint32_t rel, uint64_t &addr, uint32_t &lim, uint32_t &sep) const
	{
		if (rel < b1) {
			addr = a_head + rel;
			lim = b1;
			return true;
		}
		if (rel < b2) {
			addr = a_suf + (rel - b1);
			lim = b2;
			return true;
		}
		if (rel == b2) {
			sep = '\n';
			return false;
		}
		if (rel < b4) {
			addr = a_seq + (rel - b2 - 1);
			lim = b4;
			return true;
		}
		if (FASTQ) {
			const uint32_t b5 = b4 + 3, b6 = b5 + (b4 - b2 - 1);
			if (rel >= b5 && rel < b6) {
				addr = a_seq + ((uint64_t)in.quals - (uint64_t)in.bases) + (rel - b5);
				lim = b6;
				return true;
			}
			sep = rel == b4 + 1 ? '+' : '\n';
			return false;
		}
		sep = '\n';
		return false;
	}
};

// coff: n + 1 output offsets, total = coff[n] > 0 (n > 0: every record holds bytes).  dst holds (total + 15) / 16 16-byte vectors,
// the pad of the last one is written as 0.  marker: 0, or the byte that replaces the first byte of every header that is not empty.
template <bool FASTQ>
__global__ __launch_bounds__(kEmitBlock) void k_fmt_gather(FmtIn in, const uint64_t *__restrict__ coff, uint32_t n, uint64_t total, uint32_t marker,
                                                           uint4 *__restrict__ dst)
{
	__shared__ uint64_t range[2];
	const int tid = (int)threadIdx.x, lane = emitk::lane_id(), wave = tid / kWave;
	const uint64_t n_tiles = (total + kEmitTile - 1) / kEmitTile;
	for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const uint64_t lo = t * kEmitTile, hi = lo + kEmitTile < total ? lo + kEmitTile : total;
		// records [r0, r1) intersect [lo, hi): r0 = the first record that ends behind lo, r1 = the first that starts at or behind hi
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
			uint64_t r = emitk::owner_of(coff, r0, r1, pos);
			FmtRec<FASTQ> R;
			R.load(in, coff, r);
			uint32_t v[4];
#pragma unroll
			for (int d = 0; d < 4; ++d) {
				const uint64_t p = pos + 4u * d;
				uint32_t x = 0;
				uint64_t addr = 0;
				uint32_t lim = 0, sep = 0;
				bool whole = false; // the dword lies inside one source piece of the current record
				if (p + 4 <= R.e && p < hi) { // (p >= R.c0: every path below leaves the record that holds the byte in front of p, or a later p >= hi)
					const uint32_t rel = (uint32_t)(p - R.c0);
					whole = R.piece(in, rel, addr, lim, sep) && rel + 4 <= lim;
					if (whole) {
						x = pairk::load_unaligned_at(addr);
						if (marker && rel == 0 && R.b1) x = (x & ~0xFFu) | marker; // (the first byte of a header that is not empty)
					}
				}
				if (!whole) {
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						const uint64_t q = p + k;
						if (q >= hi) break; // behind the text: the pad stays 0 (a tile ends on a dword unless the text ends in it)
						if (q >= R.e) {     // no record is empty: the next one holds the byte
							r += 1;
							R.load(in, coff, r);
						}
						const uint32_t rel = (uint32_t)(q - R.c0);
						uint32_t b;
						if (R.piece(in, rel, addr, lim, sep)) b = (marker && rel == 0 && R.b1) ? marker : (uint32_t)*reinterpret_cast<const uint8_t *>(addr);
						else b = sep;
						x |= b << (8 * k);
					}
				}
				v[d] = x;
			}
			dst[pos >> 4] = uint4{v[0], v[1], v[2], v[3]};
		}
		__syncthreads(); // the range is rewritten by the next round
	}
}

} // namespace fmtk
} // namespace dbgk
