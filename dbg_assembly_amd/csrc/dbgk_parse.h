// PARSE stage: the bytes of a FASTQ / FASTA file, as they are, become the compact batch the other stages read in place (bases back to
// back, qualities back to back, n + 1 offsets; the layout dbgk_emit.h writes).  The record rule is the one of both host readers
// (host/reads_io.h, host/clean_common.h: RecordBatch::fill; DBG_contig/DBGgraph.cpp:244-272, clean_illumina/clean_adapter.cpp:376-387):
// a state machine over LINES -- 0 look for a header, 1 sequence, 2 separator, 3 quality -- in which only state 0 looks at what a line
// holds.  A quality line that begins with '@' is therefore told from a header by its position alone, and the state of a line is
// the composition of the transition maps of all lines in front of it: a scan.  Host side: dbgk_host_parse.h.
//
//   k_parse_count       a workgroup takes a tile of kTextTile bytes, a lane one 16-byte vector: the newline bytes per tile
//   (scan)              tile counts -> the index of the first newline of every tile (dbgk_sort.hip, rocPRIM)
//   k_parse_lines       the same loads again: the newline behind line i writes entry i + 1 of the line table -- the 31-bit start of
//                       the line, bit 31: the line is not empty and begins with the marker.  Entry 0 is line 0; the entry behind the
//                       last newline is the unterminated last line, or the end of the text.  A tile without a newline writes nothing,
//                       a line that straddles tiles is one entry like any other: nothing is carried from tile to tile but the scan.
//   k_parse_map_reduce  every line is one of two maps {0..3} -> {0..3} in one byte (2 bits per state), chosen by the marker bit.  A
//                       thread composes kLinesPerThread of them, a wave scans by shuffles, a workgroup through LDS: one map per
//                       kLineChunk lines.
//   k_parse_map_spine   ONE workgroup scans those maps, 256 at a time with a carry: the state every chunk is entered in.
//   k_parse_states      the scan inside each chunk again, from its entry state: flag[i] = line i is entered in state 0 and carries
//                       the marker bit, i.e. it is the header of a record; ignored lines counted, the last header kept.
//   (scan)              flags -> the rank of every record
//   k_parse_records     the thread of a header line writes the dbgk_parse_rec, the record's output length and the source
//                       positions of its two lines in the text; run as the length kernel of the output stage (emit_run).
//   (gather)            k_emit_gather<false, false> once per plane, source = the text (dbgk_host_emit.h, split_src)
//
// No kernel waits for another workgroup: every hand-over between workgroups is the end of a launch.
//
// Memory read: the text in whole 16-byte vectors up to n_bytes rounded up to 16; a byte at or behind n_bytes is masked out of
// the newline bits, is never tested for the marker and lies in no line, so the gather never copies it.
#pragma once

#include "dbgk_emit.h"

namespace dbgk {
namespace parsek {

using emitk::kWave;
using emitk::lane_id;

constexpr int kParseBlock = 256;
constexpr int kParseWaves = kParseBlock / kWave;
constexpr int kTextTile = kParseBlock * 16;
constexpr int kLinesPerThread = 8;
constexpr int kLineChunk = kParseBlock * kLinesPerThread;
constexpr uint32_t kMarkerBit = 1u << 31;
static_assert(DBGK_PARSE_TEXT_TILE == kTextTile, "one 16-byte load per lane reads a tile");
static_assert(kParseBlock == emitk::kEmitBlock, "k_parse_records is launched as the output stage's length kernel");

enum Counter { PC_MISMATCHED = 0, PC_SUMS, PC_MAX_LEN = PC_SUMS, PC_COUNT };

struct ParseMisc {
	unsigned long long ignored;   // lines met in state 0 without the marker bit
	unsigned long long last_head; // (index + 1) << 32 | start of the last header line; 0: none
	uint32_t final_state;         // the state behind the last line
	uint32_t pad;
};

// bit b: byte b of v is '\n', for b < valid
__device__ __forceinline__ uint32_t newline_bits(const uint4 &v, uint32_t valid)
{
	const uint32_t w[4] = {v.x, v.y, v.z, v.w};
	uint32_t m = 0;
#pragma unroll
	for (int d = 0; d < 4; ++d) {
		const uint32_t y = w[d] ^ 0x0A0A0A0Au; // a zero byte where the text holds '\n'
		const uint32_t nz = ((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y;
		const uint32_t z = (~nz & 0x80808080u) >> 7; // bits 0, 8, 16, 24
		m |= ((z * 0x00204081u >> 21) & 0xFu) << (4 * d); // ... to bits 0..3 (the partial products share no bit: no carry)
	}
	return valid >= 16 ? m : m & ((1u << valid) - 1u);
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v)
{
	for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
	return v;
}

// tile_count[t] for t < n_tiles, 0 at t == n_tiles (the scan runs over n_tiles + 1 entries, its last output is the total)
__global__ __launch_bounds__(kParseBlock) void k_parse_count(const uint4 *__restrict__ text, uint32_t n_bytes, uint32_t n_tiles,
                                                             uint32_t *__restrict__ tile_count)
{
	__shared__ uint32_t part[kParseWaves];
	const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid / kWave;
	for (uint32_t t = blockIdx.x; t <= n_tiles; t += gridDim.x) {
		if (t == n_tiles) {
			if (tid == 0) tile_count[t] = 0;
			break;
		}
		const uint32_t pos = t * (uint32_t)kTextTile + 16u * tid;
		uint32_t c = 0;
		if (pos < n_bytes) c = __popc(newline_bits(text[pos >> 4], n_bytes - pos));
		c = wave_sum32(c);
		if (lane == 0) part[wave] = c;
		__syncthreads();
		if (tid == 0) tile_count[t] = part[0] + part[1] + part[2] + part[3];
		__syncthreads(); // part is rewritten by the next round
	}
}

// tile_off: the exclusive scan of the tile counts.  table: one entry more than the text has newlines.
__global__ __launch_bounds__(kParseBlock) void k_parse_lines(const uint8_t *__restrict__ text, uint32_t n_bytes, uint32_t n_tiles,
                                                             const uint64_t *__restrict__ tile_off, uint32_t marker, uint32_t *__restrict__ table)
{
	__shared__ uint32_t part[kParseWaves];
	const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid / kWave;
	if (blockIdx.x == 0 && tid == 0) table[0] = text[0] == marker ? kMarkerBit : 0u; // line 0 (n_bytes > 0)
	for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const uint32_t pos = t * (uint32_t)kTextTile + 16u * tid;
		uint32_t m = 0;
		if (pos < n_bytes) m = newline_bits(*reinterpret_cast<const uint4 *>(text + pos), n_bytes - pos);
		const uint32_t c = __popc(m);
		uint32_t incl = c; // newlines of the lanes up to this one
		for (int d = 1; d < kWave; d <<= 1) {
			const uint32_t o = __shfl_up(incl, d, kWave);
			if (lane >= d) incl += o;
		}
		if (lane == kWave - 1) part[wave] = incl;
		__syncthreads();
		uint32_t idx = (uint32_t)tile_off[t] + incl - c;
		for (int w = 0; w < wave; ++w) idx += part[w];
		while (m) {
			const uint32_t p = pos + (uint32_t)__ffs((int)m); // the byte behind the newline: where line idx + 1 starts
			m &= m - 1;
			const bool mark = p < n_bytes && text[p] == marker;
			table[++idx] = p | (mark ? kMarkerBit : 0u);
		}
		__syncthreads(); // part is rewritten by the next round
	}
}

// ---- the maps ---------------------------------------------------------------------------------------------------------------------------
// f(s) in bits 2 s, 2 s + 1.  FASTQ: a line with the marker 0 -> 1, without 0 -> 0, and 1 -> 2 -> 3 -> 0 whatever the line holds;
// FASTA: 0 -> 1 with the marker, everything else -> 0.
constexpr uint32_t kIdentity = 0xE4;
__device__ __forceinline__ uint32_t map_of(uint32_t entry, bool fastq) { return (fastq ? 0x38u : 0x00u) | (entry >> 31); }
__device__ __forceinline__ uint32_t apply(uint32_t f, uint32_t s) { return (f >> (2 * s)) & 3u; }
// first f, then g
__device__ __forceinline__ uint32_t compose(uint32_t f, uint32_t g)
{
	return apply(g, apply(f, 0)) | apply(g, apply(f, 1)) << 2 | apply(g, apply(f, 2)) << 4 | apply(g, apply(f, 3)) << 6;
}

// The maps of one workgroup's threads, in thread order -> the composition of those in front of this thread; total: of all of them.
// Every thread of the workgroup calls it (it holds barriers).
__device__ __forceinline__ uint32_t block_scan_maps(uint32_t f, uint32_t &total)
{
	__shared__ uint32_t agg[kParseWaves];
	const int lane = lane_id(), wave = (int)threadIdx.x / kWave;
	uint32_t incl = f;
	for (int d = 1; d < kWave; d <<= 1) {
		const uint32_t o = __shfl_up(incl, d, kWave);
		if (lane >= d) incl = compose(o, incl);
	}
	__syncthreads(); // (a caller in a loop: agg of the round before has been read)
	if (lane == kWave - 1) agg[wave] = incl;
	__syncthreads();
	uint32_t excl = __shfl_up(incl, 1, kWave);
	if (lane == 0) excl = kIdentity;
	uint32_t front = kIdentity;
	total = kIdentity;
#pragma unroll
	for (int w = 0; w < kParseWaves; ++w) {
		if (w < wave) front = compose(front, agg[w]);
		total = compose(total, agg[w]);
	}
	return compose(front, excl);
}

// the maps of lines [j0, j0 + kLinesPerThread) composed; lines at and behind n_lines are the identity
__device__ __forceinline__ uint32_t thread_map(const uint32_t *__restrict__ table, uint64_t j0, uint64_t n_lines, bool fastq)
{
	uint32_t f = kIdentity;
#pragma unroll
	for (int i = 0; i < kLinesPerThread; ++i)
		if (j0 + i < n_lines) f = compose(f, map_of(table[j0 + i], fastq));
	return f;
}

// one workgroup per kLineChunk lines; agg[chunk] = the composition of the chunk's maps
__global__ __launch_bounds__(kParseBlock) void k_parse_map_reduce(const uint32_t *__restrict__ table, uint32_t n_lines, uint32_t fastq,
                                                                  uint8_t *__restrict__ agg)
{
	const uint64_t j0 = (uint64_t)blockIdx.x * kLineChunk + (uint64_t)threadIdx.x * kLinesPerThread;
	uint32_t total;
	(void)block_scan_maps(thread_map(table, j0, n_lines, fastq != 0), total);
	if (threadIdx.x == 0) agg[blockIdx.x] = (uint8_t)total;
}

// ONE workgroup: entry[c] = the state chunk c is entered in, misc->final_state = the state behind the last chunk
__global__ __launch_bounds__(kParseBlock) void k_parse_map_spine(const uint8_t *__restrict__ agg, uint32_t n_chunks, uint8_t *__restrict__ entry,
                                                                 ParseMisc *__restrict__ misc)
{
	uint32_t carry = kIdentity;
	for (uint32_t base = 0; base < n_chunks; base += kParseBlock) {
		const uint32_t c = base + threadIdx.x;
		uint32_t total;
		const uint32_t front = block_scan_maps(c < n_chunks ? (uint32_t)agg[c] : kIdentity, total);
		if (c < n_chunks) entry[c] = (uint8_t)apply(compose(carry, front), 0);
		carry = compose(carry, total);
	}
	if (threadIdx.x == 0) misc->final_state = apply(carry, 0);
}

// flag[j] for j < n_lines, 0 at j == n_lines (the grid covers n_lines + 1 entries)
__global__ __launch_bounds__(kParseBlock) void k_parse_states(const uint32_t *__restrict__ table, uint32_t n_lines, uint32_t fastq,
                                                              const uint8_t *__restrict__ entry, uint32_t *__restrict__ flag,
                                                              ParseMisc *__restrict__ misc)
{
	const uint64_t j0 = (uint64_t)blockIdx.x * kLineChunk + (uint64_t)threadIdx.x * kLinesPerThread;
	uint32_t total;
	const uint32_t front = block_scan_maps(thread_map(table, j0, n_lines, fastq != 0), total);
	uint32_t s = apply(front, entry[blockIdx.x]);
	uint32_t ignored = 0;
	unsigned long long last_head = 0;
#pragma unroll
	for (int i = 0; i < kLinesPerThread; ++i) {
		const uint64_t j = j0 + i;
		if (j > n_lines) break;
		if (j == n_lines) {
			flag[j] = 0;
			break;
		}
		const uint32_t e = table[j];
		const bool head = s == 0 && (e & kMarkerBit);
		flag[j] = head;
		ignored += s == 0 && !(e & kMarkerBit);
		if (head) last_head = (j + 1) << 32 | (e & ~kMarkerBit);
		s = apply(map_of(e, fastq != 0), s);
	}
	ignored = wave_sum32(ignored);
	for (int d = kWave / 2; d > 0; d >>= 1) last_head = max(last_head, (unsigned long long)__shfl_down(last_head, d, kWave));
	if (lane_id() == 0) {
		if (ignored) atomicAdd(&misc->ignored, (unsigned long long)ignored);
		if (last_head) atomicMax(&misc->last_head, last_head);
	}
}

struct ParseOut {
	dbgk_parse_rec *rec;
	uint32_t *len;  // n + 1 output lengths, the last one 0
	uint64_t *src;  // where the sequence line starts in the text
	uint64_t *qsrc; // ... and the quality line (with_quals)
};

// Line i of the text: lines [0, n_nl) end with a newline, line n_nl (if i < n_lines) is the unterminated last one; a line the text
// lacks is empty at the end of the text.
__device__ __forceinline__ void line_at(const uint32_t *__restrict__ table, uint64_t i, uint32_t n_lines, uint32_t n_nl, uint32_t n_bytes,
                                        uint32_t &pos, uint32_t &len)
{
	pos = n_bytes, len = 0;
	if (i >= n_lines) return;
	pos = table[i] & ~kMarkerBit;
	len = (i < n_nl ? (table[i + 1] & ~kMarkerBit) - 1u : n_bytes) - pos;
}

// The thread of a header line (flag set) writes record rank[line] if that is one of the n delivered: with last == 0 the record
// whose lines the chunk does not hold in full is rank n, and left out.
__global__ __launch_bounds__(kParseBlock) void k_parse_records(const uint32_t *__restrict__ table, const uint32_t *__restrict__ flag,
                                                               const uint64_t *__restrict__ rank, uint32_t n_lines, uint32_t n_nl, uint32_t n_bytes,
                                                               uint32_t n, uint32_t fastq, uint32_t with_quals, ParseOut o,
                                                               unsigned long long *__restrict__ counters)
{
	uint32_t mismatched = 0, longest = 0;
	const uint64_t stride = (uint64_t)gridDim.x * kParseBlock;
#pragma unroll 1
	for (uint64_t j = (uint64_t)blockIdx.x * kParseBlock + threadIdx.x; j <= n_lines; j += stride) {
		if (j == n_lines) {
			o.len[n] = 0;
			break;
		}
		if (!flag[j]) continue;
		const uint64_t r = rank[j];
		if (r >= n) continue;
		dbgk_parse_rec q;
		line_at(table, j, n_lines, n_nl, n_bytes, q.head_pos, q.head_len);
		line_at(table, j + 1, n_lines, n_nl, n_bytes, q.seq_pos, q.seq_len);
		q.qual_pos = q.qual_len = 0;
		if (fastq) line_at(table, j + 3, n_lines, n_nl, n_bytes, q.qual_pos, q.qual_len);
		uint32_t m = q.seq_len;
		if (with_quals && q.seq_len != q.qual_len) {
			m = 0;
			mismatched++;
		}
		o.rec[r] = q;
		o.len[r] = m;
		o.src[r] = q.seq_pos;
		if (with_quals) o.qsrc[r] = q.qual_pos;
		longest = max(longest, m);
	}
	for (int d = kWave / 2; d > 0; d >>= 1) longest = max(longest, (uint32_t)__shfl_down(longest, d, kWave));
	if (lane_id() == 0 && longest) atomicMax(&counters[PC_MAX_LEN], (unsigned long long)longest);
	const unsigned long long v[PC_SUMS] = {mismatched};
	emitk::fold_counters(v, counters);
}

} // namespace parsek
} // namespace dbgk
