// SIMPLIFY: kernels that trace the linear paths of the contig stage's three simplification passes (include/dbgk.h, SIMPLIFY section;
// host side in dbgk_host_simplify.h, 128-bit forms in dbgk_wide_simplify.h).
//
// remove_error_tips, remove_lowCov_edges and remove_hetero_bubbles (DBG_contig/contig.cpp:281-776) call get_linear_path (:779-827) for
// every entry of a list, in list order.  A removal changes the delete flag of the path's nodes and the link records of one or two end
// nodes; a later walk sees that only when it touches one of those slots.  So every walk of a pass is traced here against the table as
// it stands when the pass begins, one thread per walk, and the host checks each trace against the slots changed since.
//
// The walk is a chain of dependent probes; nothing is shared between threads.  Lengths first (k_simp_trace, k_simp_branches write one
// row per request), then, with offsets from the host's scan over the lengths, the nodes and base codes (k_simp_fill walks again): no
// buffer of requests x cutoff.  The kernels work on the device copy of the table that dbgk_contig_set_table made.
#pragma once

#include "dbgk_contig.h"

namespace simpk {

using contigk::bit_of;
using contigk::Table;
using dbgk::Node;

constexpr int kSimpThreads = 256;

// status of a row (DBGK_TRACE_*)
enum : uint8_t { ROW_TRACED = 0, ROW_BELOW_CUTOFF = 1, ROW_ABSENT = 2, ROW_NOT_LINEAR = 3 };

struct Row {   // dbgk_trace_row
	uint32_t start, last, len, depth;
	int8_t direct;
	uint8_t mark, status, pad;
	uint32_t reserved;
};

// what the walk needs from a table of 16-byte nodes; dbgk_wide_simplify.h has the same for 32-byte nodes
struct Ops64 {
	using Tab = Table;
	using Key = uint64_t;
	static __device__ __forceinline__ Key key_at(const Tab &t, uint64_t slot) { return t.array[slot].kmer; }
	static __device__ __forceinline__ uint32_t link_at(const Tab &t, uint64_t slot, uint32_t left)
	{
		const uint64_t links = t.array[slot].links;
		return left ? (uint32_t)links : (uint32_t)(links >> 32);
	}
	static __device__ __forceinline__ bool same(const Tab &t, uint64_t slot, Key key) { return t.array[slot].kmer == key; }
	static __device__ __forceinline__ Key neighbour(const Tab &t, Key kmer, uint32_t base, uint32_t left, bool &flip)
	{
		return contigk::neighbour_key(t, kmer, base, left, flip);       // the read-out's own (k_contig_successors)
	}
	static __device__ __forceinline__ uint64_t hash(Key key) { return dbgk::hash_code(key); }
};

// exist_kmerset: the slot of `key`, t.size when it is absent or deleted -- contigk::probe_slot, the probe of k_contig_successors
template <class O>
__device__ __forceinline__ uint32_t probe(const typename O::Tab &t, typename O::Key key)
{
	return (uint32_t)contigk::probe_slot(t, O::hash(key), [&](uint64_t s) { return O::same(t, s, key); });
}

// get_linear_path (contig.cpp:779-827) from slot idx, leaving leftward (left = 1) or rightward.  The body runs before the test: a cutoff
// below 2 gives one step; the start node is walked whatever its state.  nodes / codes: where the steps' slots and base codes (in the
// orientation of the path's string) go, or null pointers in the length pass.
template <class O>
__device__ __forceinline__ void walk(const typename O::Tab &t, uint32_t idx, uint32_t left, int32_t cutoff, uint32_t *__restrict__ nodes,
                                     uint8_t *__restrict__ codes, Row &r)
{
	const uint32_t original = left;
	uint32_t len = 0, depth = 0;
	for (;;) {
		const uint32_t kl = t.klink[idx];
		const uint32_t base = left ? (kl >> 2) & 3u : (kl >> 6) & 3u;
		depth += (O::link_at(t, idx, left) >> ((3u - base) * 8u)) & 0xffu;
		if (nodes) {
			nodes[len] = idx;
			codes[len] = (uint8_t)(left == original ? base : 3u - base);
		}
		++len;
		bool flip;
		const typename O::Key key = O::neighbour(t, O::key_at(t, idx), base, left, flip);
		if (flip) left ^= 1u;
		idx = probe<O>(t, key);
		const uint32_t kv = idx == (uint32_t)t.size ? 0u : t.klink[idx];
		if (!(kv & 0x100u) || (int32_t)len >= cutoff) {
			r.last = idx;
			r.mark = (idx == (uint32_t)t.size || (kv & 3u) == 0 || ((kv >> 4) & 3u) == 0) ? 0 : 1;
			break;
		}
	}
	r.len = len;
	r.depth = depth;
}

template <class O>
__device__ __forceinline__ void trace_body(const typename O::Tab &t, const uint32_t *__restrict__ req_slot, const int8_t *__restrict__ req_direct,
                                           uint32_t n, int32_t cutoff, Row *__restrict__ rows)
{
	for (uint32_t i = blockIdx.x * kSimpThreads + threadIdx.x; i < n; i += gridDim.x * kSimpThreads) {
		Row r = {};
		r.start = req_slot[i];
		r.direct = req_direct[i];
		r.status = ROW_TRACED;
		walk<O>(t, r.start, r.direct < 0 ? 1u : 0u, cutoff, nullptr, nullptr, r);
		rows[i] = r;
	}
}

// row 8 i + 4 side + j: the edge with base j on the right (side 0) or left (side 1) of branching slot i (get_branch_bases, contig.cpp:361-370;
// the neighbour as remove_lowCov_edges and remove_hetero_bubbles find it, :640-648, :420-440).  Rows without a trace carry the
// neighbour's slot and why there is none.
template <class O>
__device__ __forceinline__ void branches_body(const typename O::Tab &t, const uint32_t *__restrict__ slots, uint32_t n_rows, int32_t cutoff,
                                              int32_t freq_cutoff, Row *__restrict__ rows)
{
	for (uint32_t i = blockIdx.x * kSimpThreads + threadIdx.x; i < n_rows; i += gridDim.x * kSimpThreads) {
		const uint32_t idx = slots[i >> 3], left = (i >> 2) & 1u, j = i & 3u;
		Row r = {};
		r.start = r.last = (uint32_t)t.size;
		const int32_t depth = (int32_t)((O::link_at(t, idx, left) >> ((3u - j) * 8u)) & 0xffu);
		if (depth <= freq_cutoff) {
			r.status = ROW_BELOW_CUTOFF;
		} else {
			bool flip;
			const typename O::Key key = O::neighbour(t, O::key_at(t, idx), j, left, flip);
			const uint32_t left_after = flip ? left ^ 1u : left;
			const uint32_t v = probe<O>(t, key);
			r.start = v;
			r.direct = left_after ? -1 : 1;
			if (v == (uint32_t)t.size) r.status = ROW_ABSENT;
			else if (!(t.klink[v] & 0x100u)) r.status = ROW_NOT_LINEAR;
			else {
				r.status = ROW_TRACED;
				walk<O>(t, v, left_after, cutoff, nullptr, nullptr, r);
			}
		}
		rows[i] = r;
	}
}

// the second pass: every traced row walks again and writes its nodes and base codes at first[i]
template <class O>
__device__ __forceinline__ void fill_body(const typename O::Tab &t, const Row *__restrict__ rows, const uint64_t *__restrict__ first, uint32_t n,
                                          int32_t cutoff, uint32_t *__restrict__ nodes, uint8_t *__restrict__ codes)
{
	for (uint32_t i = blockIdx.x * kSimpThreads + threadIdx.x; i < n; i += gridDim.x * kSimpThreads) {
		Row r = rows[i];
		if (r.len == 0) continue;
		// the table has not changed since the length pass, so this is the same walk; bounding it by the length it had keeps every store
		// inside the row's [first[i], first[i] + len) whatever happens
		walk<O>(t, r.start, r.direct < 0 ? 1u : 0u, min(cutoff, (int32_t)r.len), nodes + first[i], codes + first[i], r);
	}
}

__global__ __launch_bounds__(kSimpThreads) void k_simp_trace(Table t, const uint32_t *__restrict__ req_slot, const int8_t *__restrict__ req_direct,
                                                             uint32_t n, int32_t cutoff, Row *__restrict__ rows)
{
	trace_body<Ops64>(t, req_slot, req_direct, n, cutoff, rows);
}

__global__ __launch_bounds__(kSimpThreads) void k_simp_branches(Table t, const uint32_t *__restrict__ slots, uint32_t n_rows, int32_t cutoff,
                                                                int32_t freq_cutoff, Row *__restrict__ rows)
{
	branches_body<Ops64>(t, slots, n_rows, cutoff, freq_cutoff, rows);
}

__global__ __launch_bounds__(kSimpThreads) void k_simp_fill(Table t, const Row *__restrict__ rows, const uint64_t *__restrict__ first, uint32_t n,
                                                            int32_t cutoff, uint32_t *__restrict__ nodes, uint8_t *__restrict__ codes)
{
	fill_body<Ops64>(t, rows, first, n, cutoff, nodes, codes);
}

// Host-side changes into the device copy: the two link words and the link record of n slots (no slot twice), and n_bytes bytes of the
// delete flags (no byte twice: two slots of one byte never race).  The link words of slot s lie at array + s * node_bytes + link_off,
// for both kinds of node.
__global__ __launch_bounds__(kSimpThreads) void k_simp_update(uint8_t *__restrict__ array, uint32_t node_bytes, uint32_t link_off,
                                                              uint16_t *__restrict__ klink, uint8_t *__restrict__ del, const uint32_t *__restrict__ slots,
                                                              const uint2 *__restrict__ links, const uint16_t *__restrict__ records, uint32_t n,
                                                              const uint32_t *__restrict__ byte_at, const uint8_t *__restrict__ byte_val, uint32_t n_bytes)
{
	const uint32_t m = n > n_bytes ? n : n_bytes;
	for (uint32_t i = blockIdx.x * kSimpThreads + threadIdx.x; i < m; i += gridDim.x * kSimpThreads) {
		if (i < n) {
			const uint32_t s = slots[i];
			*reinterpret_cast<uint2 *>(array + (uint64_t)s * node_bytes + link_off) = links[i];   // 8-byte aligned in both node layouts
			klink[s] = records[i];
		}
		if (i < n_bytes) del[byte_at[i]] = byte_val[i];
	}
}

} // namespace simpk
