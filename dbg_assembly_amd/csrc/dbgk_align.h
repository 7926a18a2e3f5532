// dbgk_align.h -- ALIGN: the global alignments of the contig stage's bubble arms, many independent pairs at once (gfx950 only;
// include/dbgk.h, SIMPLIFY section).
//
// Reference semantics (DBG_contig/global_aligning.cpp):
//   global_aligning   :98-182   Needleman-Wunsch, match 3, mismatch -5, gap -5, int scores; row 0 is -5 j with direction 1, column 0 is
//                               -5 i with direction 2
//   get_max_score     :20-35    direction 0 (substitution) if sub >= gapi && sub >= gapj, else 1 (gap in seq_i) if gapi > sub &&
//                               gapi >= gapj, else 2 (gap in seq_j)
//   trace_back        :39-68    from (len_i, len_j) until both positions are 0, then both strings reversed
//
// k_align_pairs keeps no matrix of scores: one wave per pair, rows in strips of 64, lane l owns row r0 + l + 1 of the strip and sweeps
// it skewed by its lane number, so the wave works on one anti-diagonal per step.  A cell needs its left neighbour (the lane's own last
// score), the cell above (the score the lane above computed one step earlier, moved down one lane) and the one diagonally above (what
// came down the step before); the character of seq_j travels down the lanes the same way.  Lane 0 takes the row above its strip and
// the next character from LDS, lane 63 leaves its row there for the next strip.  Only the directions are stored: 2 bits per cell,
// 16 cells to a dword, every lane writing the dwords of its own row, rows kAlignRowWords = 17 dwords apart -- the lanes that finish a
// dword in the same step are 16 rows apart, which an odd stride puts on distinct banks.  Lane 0 then follows the directions back (at most
// len_i + len_j dependent LDS reads) and leaves the alignment reversed in LDS; the wave writes it out forwards.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dbgk {
namespace alignk {

constexpr uint32_t kAlignMaxLen = 256;                     // == DBGK_ALIGN_MAX_LEN: longest sequence of a pair
constexpr uint32_t kAlignRowWords = kAlignMaxLen / 16 + 1; // dwords of directions per row, and one to make the stride odd
constexpr int kAlignThreads = 64;                          // one wave, one pair at a time
constexpr int32_t kMatch = 3, kMismatch = -5, kGap = -5;

struct Row { // == dbgk_align_row
	uint32_t len_i, len_j;
	int32_t score;
	uint32_t aligned_len, diffs;
	uint8_t status, pad[3];
};

struct AlignLds { // 19992 bytes: eight workgroups to a CU of 160 KiB
	uint32_t dir[kAlignMaxLen * kAlignRowWords]; // direction of cell (i, j), i, j >= 1: bits 2 ((j - 1) & 15) of dir[(i - 1) * 17 + ((j - 1) >> 4)]
	int32_t edge[kAlignMaxLen + 4];              // scores of the row above the strip, columns 0 .. len_j
	uint8_t si[kAlignMaxLen], sj[kAlignMaxLen];
	uint8_t out_i[2 * kAlignMaxLen], out_j[2 * kAlignMaxLen]; // the alignment from its last column to its first
	int32_t score;
	uint32_t columns;
};
static_assert(sizeof(AlignLds) <= 64 * 1024, "static LDS: no attribute call");

// the value of the lane one below in number (lane 0 gets 0): DPP wave_shr:1, one VALU instruction
__device__ __forceinline__ int32_t from_lane_above(int32_t v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, false); }

// pair p = sequences 2 p and 2 p + 1 of seqs (off: 2 n_pairs + 1 entries); its aligned strings go to out_i / out_j from out_off[p], which
// leaves it len_i + len_j bytes in each.  A pair with a sequence longer than kAlignMaxLen, or an empty one, is not aligned.
__global__ __launch_bounds__(kAlignThreads) void k_align_pairs(const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off, uint32_t n_pairs,
                                                               const uint64_t *__restrict__ out_off, Row *__restrict__ rows,
                                                               uint8_t *__restrict__ out_i, uint8_t *__restrict__ out_j)
{
	__shared__ AlignLds L;
	const uint32_t lane = threadIdx.x;
	for (uint32_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
		const uint64_t oi = off[2 * p], oj = off[2 * p + 1], oe = off[2 * p + 2];
		if (oj - oi > kAlignMaxLen || oe - oj > kAlignMaxLen || oj == oi || oe == oj) { // the host sends no such pair
			if (lane == 0) rows[p] = Row{(uint32_t)(oj - oi), (uint32_t)(oe - oj), 0, 0u, 0u, 1, {0, 0, 0}};
			continue;
		}
		const uint32_t ni = (uint32_t)(oj - oi), nj = (uint32_t)(oe - oj);
		__syncthreads(); // the pair before has been written out
		for (uint32_t x = lane; x < ni; x += kAlignThreads) L.si[x] = seqs[oi + x];
		for (uint32_t x = lane; x < nj; x += kAlignThreads) L.sj[x] = seqs[oj + x];
		for (uint32_t x = lane; x <= nj; x += kAlignThreads) L.edge[x] = kGap * (int32_t)x;
		__syncthreads();
		for (uint32_t r0 = 0; r0 < ni; r0 += kAlignThreads) {
			const uint32_t i = r0 + lane + 1; // this lane's row
			const bool row_ok = i <= ni;
			const uint32_t a = L.si[min(i, ni) - 1];
			uint32_t *const dir_row = L.dir + (min(i, ni) - 1) * kAlignRowWords;
			int32_t left = kGap * (int32_t)i, diag = kGap * (int32_t)(i - 1), b = 0;
			uint32_t acc = 0;
			// what lane 0 needs at step 1: the score above column 1 and the character of column 1
			int32_t edge_next = L.edge[1], b_next = L.sj[0];
			const uint32_t steps = nj + min((uint32_t)kAlignThreads, ni - r0) - 1;
			for (uint32_t t = 1; t <= steps; ++t) {
				int32_t up = from_lane_above(left);
				b = from_lane_above(b);
				if (lane == 0) {
					up = edge_next;
					b = b_next;
				}
				edge_next = L.edge[min(t + 1, nj)]; // the same address in every lane; lane 63 is 63 columns behind with its stores
				b_next = L.sj[min(t, nj - 1)];
				const uint32_t j = t - lane; // this lane's column
				if (row_ok && j - 1u < nj) {
					const int32_t sub = diag + ((uint32_t)b == a ? kMatch : kMismatch), gapi = left + kGap, gapj = up + kGap;
					uint32_t d;
					int32_t best;
					if (sub >= gapi && sub >= gapj) best = sub, d = 0;
					else if (gapi > sub && gapi >= gapj) best = gapi, d = 1;
					else best = gapj, d = 2;
					diag = up;
					left = best;
					acc |= d << (2u * ((j - 1u) & 15u));
					if (((j - 1u) & 15u) == 15u || j == nj) {
						dir_row[(j - 1u) >> 4] = acc;
						acc = 0;
					}
					if (lane == kAlignThreads - 1) L.edge[j] = best;
					if (i == ni && j == nj) L.score = best;
				}
			}
			__syncthreads(); // the strip's last row and its directions are in LDS
		}
		if (lane == 0) { // trace_back
			uint32_t i = ni, j = nj, n = 0, diffs = 0;
			do {
				uint32_t d;
				if (i == 0) d = 1;
				else if (j == 0) d = 2;
				else d = (L.dir[(i - 1) * kAlignRowWords + ((j - 1) >> 4)] >> (2u * ((j - 1) & 15u))) & 3u;
				uint8_t ci = '-', cj = '-';
				if (d != 1) ci = L.si[--i];
				if (d != 2) cj = L.sj[--j];
				L.out_i[n] = ci;
				L.out_j[n] = cj;
				diffs += (ci != cj && ci != '-' && cj != '-') ? 1u : 0u;
				++n;
			} while (i > 0 || j > 0);
			L.columns = n;
			rows[p] = Row{ni, nj, L.score, n, diffs, 0, {0, 0, 0}};
		}
		__syncthreads();
		const uint32_t n = L.columns; // <= ni + nj
		const uint64_t oo = out_off[p];
		for (uint32_t x = lane; x < n; x += kAlignThreads) {
			out_i[oo + x] = L.out_i[n - 1 - x];
			out_j[oo + x] = L.out_j[n - 1 - x];
		}
	}
}

} // namespace alignk
} // namespace dbgk
