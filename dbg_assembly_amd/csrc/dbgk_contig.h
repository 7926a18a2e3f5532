// CONTIG: kernels of the contig read-out on the GPU (include/dbgk.h, CONTIG section; host side in dbgk_host_contig.h).
//
// The reference reads contigs out with a serial scan in slot order (DBG_contig/contig.cpp:900-1011): at the first live linear node it
// walks right, then left (get_linear_seq, :832-896), deleting what it passes.  Here the live linear nodes are numbered in slot order
// ("dense" index i, port 2 i = leaving rightward, port 2 i + 1 = leaving leftward), every port finds the port its walk continues
// through (k_contig_successors), steps that are not answered by the neighbour's link back are cut and both nodes marked
// (k_contig_mutual), and pointer jumping over the ports (k_contig_jump) gives every port the number of nodes, the depth sum, the
// smallest node and the OR of the marks from itself to the end of its walk.  A chain without a mark that is no cycle is read out
// from its smallest node (the anchor, where the reference's scan meets it first); every other chain is handed to the host walker.
#pragma once

#include "dbgk_device.h"

namespace contigk {

using dbgk::ModMagic;
using dbgk::Node;

constexpr int kContigThreads = 256;
constexpr int kScanItems = 8;                          // items per thread of the two ordered compactions
constexpr uint32_t kScanTile = kContigThreads * kScanItems;
constexpr uint32_t kEnd = 0xffffffffu;                 // no next port / no slot
constexpr uint32_t kMarkBit = 0x80000000u;             // in PortState::dist: a marked node lies on the span
constexpr uint32_t kDistMask = 0x7fffffffu;

// end classes of a step (get_linear_seq, contig.cpp:873-890)
enum : uint32_t { END_NONE = 0, END_ABSENT = 1, END_BREAK_NODE = 2, END_UNIQUE = 3, END_REPEAT = 4 };

struct Table {
	const Node *array;
	const uint8_t *nul, *del;
	const uint16_t *klink;
	uint64_t size;
	ModMagic magic;
	int k;
};

// what pointer jumping carries per port, over the span from the port to where its pointer stands
struct alignas(16) PortState {
	uint32_t next;      // port the walk continues through behind the span, kEnd when the span reaches the end of the walk
	uint32_t dist;      // nodes on the span (saturating at kDistMask: only cycles get there) | kMarkBit
	uint32_t sum;       // sum of the steps' depths
	uint32_t minp;      // port of the span's node with the smallest dense index
};

struct alignas(16) Record {   // dbgk_contig_record
	uint64_t anchor, left_end, right_end;
	uint32_t left_len, right_len, left_depth, right_depth;
	uint8_t left_mark, right_mark, left_repeat, right_repeat, host_walked, mid_depth, pad[2];
};

__device__ __forceinline__ bool bit_of(const uint8_t *flags, uint64_t i) { return (flags[i >> 3] & (0x80u >> (i & 7u))) != 0; }   // kmerSet.h:144-169

// the nodes read_out_contig starts from and get_linear_seq walks through (contig.cpp:931, :873)
__device__ __forceinline__ bool live_linear(const Table &t, uint64_t slot)
{
	return bit_of(t.nul, slot) && !bit_of(t.del, slot) && (t.klink[slot] & 0x100u);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	return v;
}

// exclusive scan over the block's kContigThreads values; sh holds 4 values; total = the block's sum
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T *sh, T &total)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	T inc = v;
	for (uint32_t o = 1; o < 64; o <<= 1) {
		const T n = __shfl_up(inc, o, 64);
		if (lane >= o) inc += n;
	}
	__syncthreads();                 // the previous round's readers of sh are done
	if (lane == 63) sh[wave] = inc;
	__syncthreads();
	T base = 0;
	for (uint32_t w = 0; w < wave; ++w) base += sh[w];
	total = sh[0] + sh[1] + sh[2] + sh[3];
	return base + inc - v;
}

// live linear nodes per tile of kScanTile slots
__global__ __launch_bounds__(kContigThreads) void k_contig_count_linear(Table t, uint32_t *__restrict__ tile_count)
{
	__shared__ uint32_t sh[4];
	const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
	uint32_t n = 0;
	for (int it = 0; it < kScanItems; ++it) {
		const uint64_t slot = base + (uint64_t)it * kContigThreads + threadIdx.x;
		if (slot < t.size && live_linear(t, slot)) ++n;
	}
	n = wave_sum(n);
	if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = n;
	__syncthreads();
	if (threadIdx.x == 0) tile_count[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// dense numbering in slot order: slot_of[i] and dense_of[slot] (kEnd for every other slot)
__global__ __launch_bounds__(kContigThreads) void k_contig_compact_linear(Table t, const uint32_t *__restrict__ tile_first,
                                                                          uint32_t *__restrict__ slot_of, uint32_t *__restrict__ dense_of)
{
	__shared__ uint32_t sh[4];
	const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
	uint32_t running = tile_first[blockIdx.x];
	for (int it = 0; it < kScanItems; ++it) {
		const uint64_t slot = base + (uint64_t)it * kContigThreads + threadIdx.x;
		const bool in = slot < t.size;
		const uint32_t f = in && live_linear(t, slot) ? 1u : 0u;
		uint32_t total;
		const uint32_t at = running + block_excl_scan<uint32_t>(f, sh, total);
		if (f) slot_of[at] = (uint32_t)slot;
		if (in) dense_of[slot] = f ? at : kEnd;
		running += total;
	}
}

// The neighbour of `kmer` through the link with code `base` on its left or right side (contig.h:119-130) in canonical form; a
// palindrome counts as flipped (contig.cpp:802, :858).  k <= 31
__device__ __forceinline__ uint64_t neighbour_key(const Table &t, uint64_t kmer, uint32_t base, uint32_t left, bool &flip)
{
	const uint64_t nk = left ? (kmer >> 2) + ((uint64_t)base << (2 * (t.k - 1))) : ((kmer << 2) | base) & ((1ull << (2 * t.k)) - 1);
	const uint64_t rc = dbgk::revcomp_kbit(nk, t.k);
	flip = !(nk < rc);
	return flip ? rc : nk;
}

// exist_kmerset (kmerSet.cpp:280-302) on a table of either node width: the slot on the chain from hash % size for which same(slot)
// holds, t.size when the chain ends at an empty slot first or the match is deleted.  Bounded by the table size: a table without an
// empty slot ends here, not in a loop.  The one statement of the rule for the read-out's successors and the simplification walks
template <class Tab, class Same>
__device__ __forceinline__ uint64_t probe_slot(const Tab &t, uint64_t hash, Same same)
{
	uint64_t v = dbgk::fast_mod(hash, t.magic);
	for (uint64_t tries = 0; tries < t.size; ++tries) {
		if (!bit_of(t.nul, v)) break;
		if (same(v)) return bit_of(t.del, v) ? t.size : v;
		v = v + 1 == t.size ? 0 : v + 1;
	}
	return t.size;
}

// One step of get_linear_seq (contig.cpp:844-890) per port: the neighbour's k-mer, its canonical form and the direction the walk has
// behind it, the probe of exist_kmerset (kmerSet.cpp:280-302: deleted and empty slots are absent), and how the step ends.
//   raw_next[p]  port the walk continues through when the neighbour is a live linear node, kEnd otherwise
//   step[p]      base code of the link (2 bits) | its depth << 8 | end class << 16
//   end_slot[p]  the neighbour's slot (kEnd when absent)
__global__ __launch_bounds__(kContigThreads) void k_contig_successors(Table t, const uint32_t *__restrict__ slot_of,
                                                                      const uint32_t *__restrict__ dense_of, uint32_t n_ports,
                                                                      uint32_t *__restrict__ raw_next, uint32_t *__restrict__ step,
                                                                      uint32_t *__restrict__ end_slot)
{
	for (uint32_t p = blockIdx.x * kContigThreads + threadIdx.x; p < n_ports; p += gridDim.x * kContigThreads) {
		const uint32_t left = p & 1u;
		const uint64_t u = slot_of[p >> 1];
		const Node nd = t.array[u];
		const uint32_t kl = t.klink[u];
		const uint32_t base = left ? (kl >> 2) & 3u : (kl >> 6) & 3u;
		const uint32_t link = left ? (uint32_t)nd.links : (uint32_t)(nd.links >> 32);
		const uint32_t depth = (link >> ((3u - base) * 8u)) & 0xffu;
		bool flip;
		const uint64_t key = neighbour_key(t, nd.kmer, base, left, flip);
		const uint64_t v = probe_slot(t, dbgk::hash_code(key), [&](uint64_t s) { return t.array[s].kmer == key; });
		const bool found = v != t.size;
		uint32_t cls = END_ABSENT, nxt = kEnd, es = kEnd;
		if (found) {
			const uint32_t kv = t.klink[v];
			const uint32_t left_after = flip ? left ^ 1u : left;        // the walk's direction at the neighbour
			es = (uint32_t)v;
			if (kv & 0x100u) {
				cls = END_NONE;
				nxt = 2u * dense_of[v] + left_after;
			} else {
				const uint32_t vl = kv & 3u, vr = (kv >> 4) & 3u;
				if (vl == 0 || vr == 0) cls = END_BREAK_NODE;
				else cls = (left_after ? vl > 1 : vr > 1) ? END_REPEAT : END_UNIQUE;
			}
		}
		raw_next[p] = nxt;
		step[p] = base | (depth << 8) | (cls << 16);
		end_slot[p] = es;
	}
}

// A step p -> q between linear nodes is mutual when the walk that leaves q's node the other way continues through p's node the
// other way (port q ^ 1 leads to port p ^ 1).  Steps that are not, and steps of a node onto itself, are cut and mark both nodes.
__global__ __launch_bounds__(kContigThreads) void k_contig_mutual(const uint32_t *__restrict__ raw_next, uint32_t n_ports,
                                                                  uint32_t *__restrict__ next, uint32_t *__restrict__ mark)
{
	for (uint32_t p = blockIdx.x * kContigThreads + threadIdx.x; p < n_ports; p += gridDim.x * kContigThreads) {
		uint32_t q = raw_next[p];
		if (q != kEnd && (raw_next[q ^ 1u] != (p ^ 1u) || (q >> 1) == (p >> 1))) {
			mark[p >> 1] = 1u;
			mark[q >> 1] = 1u;
			q = kEnd;
		}
		next[p] = q;
	}
}

__global__ __launch_bounds__(kContigThreads) void k_contig_rank_init(const uint32_t *__restrict__ next, const uint32_t *__restrict__ mark,
                                                                     const uint32_t *__restrict__ step, uint32_t n_ports,
                                                                     PortState *__restrict__ st)
{
	for (uint32_t p = blockIdx.x * kContigThreads + threadIdx.x; p < n_ports; p += gridDim.x * kContigThreads) {
		PortState s;
		s.next = next[p];
		s.dist = 1u | (mark[p >> 1] ? kMarkBit : 0u);
		s.sum = (step[p] >> 8) & 0xffu;
		s.minp = p;
		st[p] = s;
	}
}

// one round of pointer jumping: the span of p grows by the span of the port its pointer stands on
__global__ __launch_bounds__(kContigThreads) void k_contig_jump(const PortState *__restrict__ in, uint32_t n_ports, PortState *__restrict__ out)
{
	for (uint32_t p = blockIdx.x * kContigThreads + threadIdx.x; p < n_ports; p += gridDim.x * kContigThreads) {
		PortState s = in[p];
		if (s.next != kEnd) {
			const PortState n = in[s.next];
			const uint32_t d = (s.dist & kDistMask) + (n.dist & kDistMask);
			s.dist = (d > kDistMask ? kDistMask : d) | ((s.dist | n.dist) & kMarkBit);
			s.sum += n.sum;
			s.minp = (n.minp >> 1) < (s.minp >> 1) ? n.minp : s.minp;
			s.next = n.next;
		}
		out[p] = s;
	}
}

// Per node: host (its chain holds a marked node, or it is on a cycle: a pointer that has not reached an end after the last round),
// anchor (the smallest node of a chain the kernels read out; alen = bytes of its contig) or neither.  Per tile: anchors and bytes.
__global__ __launch_bounds__(kContigThreads) void k_contig_classify(const PortState *__restrict__ st, uint32_t n_nodes, int k,
                                                                    uint32_t *__restrict__ alen, uint8_t *__restrict__ host_flag,
                                                                    uint32_t *__restrict__ tile_count, uint64_t *__restrict__ tile_bytes)
{
	__shared__ uint32_t shc[4];
	__shared__ uint64_t shb[4];
	const uint32_t base = blockIdx.x * kScanTile;
	uint32_t cnt = 0;
	uint64_t bytes = 0;
	for (int it = 0; it < kScanItems; ++it) {
		const uint32_t i = base + it * kContigThreads + threadIdx.x;
		if (i >= n_nodes) continue;
		const PortState r = st[2 * i], l = st[2 * i + 1];
		const bool host = r.next != kEnd || l.next != kEnd || ((r.dist | l.dist) & kMarkBit);
		const uint32_t amin = min(r.minp >> 1, l.minp >> 1);
		const uint32_t len = !host && amin == i ? (l.dist & kDistMask) + (uint32_t)k + (r.dist & kDistMask) : 0u;
		alen[i] = len;
		host_flag[i] = host ? 1 : 0;
		cnt += len ? 1u : 0u;
		bytes += len;
	}
	cnt = wave_sum(cnt);
	for (int o = 32; o > 0; o >>= 1) bytes += __shfl_down(bytes, o, 64);
	if ((threadIdx.x & 63u) == 0) {
		shc[threadIdx.x >> 6] = cnt;
		shb[threadIdx.x >> 6] = bytes;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		tile_count[blockIdx.x] = shc[0] + shc[1] + shc[2] + shc[3];
		tile_bytes[blockIdx.x] = shb[0] + shb[1] + shb[2] + shb[3];
	}
}

// contigs in anchor order: contig_of[anchor], the contig's first byte and the anchor's half of its record
__global__ __launch_bounds__(kContigThreads) void k_contig_place(const PortState *__restrict__ st, const uint32_t *__restrict__ alen,
                                                                 const uint32_t *__restrict__ slot_of, uint32_t n_nodes,
                                                                 const uint32_t *__restrict__ tile_first, const uint64_t *__restrict__ tile_byte0,
                                                                 uint32_t *__restrict__ contig_of, uint64_t *__restrict__ ctg_off,
                                                                 Record *__restrict__ rec)
{
	__shared__ uint32_t shc[4];
	__shared__ uint64_t shb[4];
	const uint32_t base = blockIdx.x * kScanTile;
	uint32_t run_c = tile_first[blockIdx.x];
	uint64_t run_b = tile_byte0[blockIdx.x];
	for (int it = 0; it < kScanItems; ++it) {
		const uint32_t i = base + it * kContigThreads + threadIdx.x;
		const uint32_t len = i < n_nodes ? alen[i] : 0u;
		uint32_t tc;
		uint64_t tb;
		const uint32_t c = run_c + block_excl_scan<uint32_t>(len ? 1u : 0u, shc, tc);
		const uint64_t b = run_b + block_excl_scan<uint64_t>(len, shb, tb);
		if (len) {
			const PortState r = st[2 * i], l = st[2 * i + 1];
			contig_of[i] = c;
			ctg_off[c] = b;
			Record x = {};
			x.anchor = slot_of[i];
			x.left_len = l.dist & kDistMask;
			x.right_len = r.dist & kDistMask;
			x.left_depth = l.sum;
			x.right_depth = r.sum;
			// the middle k-mer's depth byte: (char)avgDepth, 10 and 62 one less (contig.cpp:980-989)
			const double avg = (double)(l.sum + r.sum) / (double)(x.left_len + x.right_len);
			uint32_t md = (uint32_t)(int)avg & 0xffu;
			if (md == 10 || md == 62) --md;
			x.mid_depth = (uint8_t)md;
			rec[c] = x;      // the end fields are written by k_contig_scatter, which runs behind this kernel
		}
		run_c += tc;
		run_b += tb;
	}
}

// Every node of a kernel chain puts its step -- base code | depth byte << 8 -- where the contig has it: the anchor's two steps on
// either side of the middle k-mer, a node j steps to the right of the anchor j bytes further right, one to the left j bytes
// further left (the reference reverses the left part, contig.cpp:974-975).  Walking away from the anchor against the side's own
// direction gives the complement base (:853, :862).  The last node of a side writes how the side ends.
__global__ __launch_bounds__(kContigThreads) void k_contig_scatter(const PortState *__restrict__ st, const uint32_t *__restrict__ step,
                                                                   const uint32_t *__restrict__ end_slot, const uint8_t *__restrict__ host_flag,
                                                                   const uint32_t *__restrict__ contig_of, const uint64_t *__restrict__ ctg_off,
                                                                   uint32_t n_nodes, int k, uint64_t table_size, uint16_t *__restrict__ stage,
                                                                   Record *__restrict__ rec)
{
	for (uint32_t i = blockIdx.x * kContigThreads + threadIdx.x; i < n_nodes; i += gridDim.x * kContigThreads) {
		if (host_flag[i]) continue;
		const PortState r = st[2 * i], l = st[2 * i + 1];
		const uint32_t a = min(r.minp >> 1, l.minp >> 1);
		const uint32_t c = contig_of[a];
		const uint64_t off = ctg_off[c];
		const uint32_t left_len = st[2 * a + 1].dist & kDistMask;
		// sides to write: the anchor both, every other node the one that leads away from the anchor
		for (uint32_t side = 0; side < 2; ++side) {          // 0: the contig's right part, 1: its left part
			uint32_t port, j;
			if (a == i) {
				port = 2 * i + side;
				j = 0;
			} else {
				const uint32_t toward = (r.minp >> 1) == a ? 0u : 1u;            // the direction at this node that leads to the anchor
				const PortState t = toward ? l : r;
				const uint32_t at_anchor = t.minp & 1u;                         // ... arrives there walking this way
				if ((at_anchor ^ 1u) != side) continue;                         // arriving leftward: this node lies to the right
				port = 2 * i + (toward ^ 1u);
				j = (t.dist & kDistMask) - (st[t.minp].dist & kDistMask);
			}
			const uint32_t s = step[port];
			uint32_t code = s & 3u, depth = (s >> 8) & 0xffu;
			if ((port & 1u) != side) code = 3u - code;
			if (depth == 10 || depth == 62) --depth;                            // contig.cpp:849-851
			const uint64_t pos = side ? off + left_len - 1 - j : off + left_len + (uint32_t)k + j;
			stage[pos] = (uint16_t)(code | (depth << 8));
			const PortState mine = (port & 1u) ? l : r;
			if ((mine.dist & kDistMask) == 1u) {                                // the side's last node
				const uint32_t cls = (s >> 16) & 7u, es = end_slot[port];
				const uint64_t end = es == kEnd ? table_size : es;
				const uint8_t mark = cls == END_UNIQUE || cls == END_REPEAT ? 1 : 0;
				const uint8_t rep = cls == END_UNIQUE ? 1 : cls == END_REPEAT ? 2 : 0;
				if (side) {
					rec[c].left_end = end;
					rec[c].left_mark = mark;
					rec[c].left_repeat = rep;
				} else {
					rec[c].right_end = end;
					rec[c].right_mark = mark;
					rec[c].right_repeat = rep;
				}
			}
		}
	}
}

// read-out: one thread writes 8 consecutive bytes of the bases and of the depths with one store each; it finds the contig of its
// first byte by bisection and moves on as it crosses contig ends.  Bytes of the middle k-mer come from the anchor's k-mer and the
// record's average-depth byte, all others from the staged steps.
__global__ __launch_bounds__(kContigThreads) void k_contig_emit(const uint16_t *__restrict__ stage, const uint64_t *__restrict__ ctg_off,
                                                                const Record *__restrict__ rec, const Node *__restrict__ array,
                                                                uint32_t n_contigs, uint64_t total, int k, uint8_t *__restrict__ bases,
                                                                uint8_t *__restrict__ depths)
{
	const uint64_t n_words = (total + 7) / 8;
	for (uint64_t w = (uint64_t)blockIdx.x * kContigThreads + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * kContigThreads) {
		const uint64_t p0 = w * 8;
		uint32_t lo = 0, hi = n_contigs;                 // the contig with ctg_off[c] <= p0 < ctg_off[c + 1] (no contig is empty)
		while (hi - lo > 1) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (ctg_off[mid] <= p0) lo = mid; else hi = mid;
		}
		uint32_t c = lo;
		uint64_t c_begin = ctg_off[c], c_end = ctg_off[c + 1];
		uint32_t left_len = rec[c].left_len, md = rec[c].mid_depth;
		uint64_t kmer = array[rec[c].anchor].kmer;
		uint64_t wb = 0, wd = 0;
		const uint32_t n_bytes = (uint32_t)(total - p0 < 8 ? total - p0 : 8);
		for (uint32_t b = 0; b < n_bytes; ++b) {
			const uint64_t p = p0 + b;
			while (p >= c_end) {
				++c;
				c_begin = c_end;
				c_end = ctg_off[c + 1];
				left_len = rec[c].left_len;
				md = rec[c].mid_depth;
				kmer = array[rec[c].anchor].kmer;
			}
			const uint64_t rel = p - c_begin;
			uint32_t code, depth;
			if (rel >= left_len && rel < left_len + (uint32_t)k) {
				code = (uint32_t)(kmer >> (2 * ((uint32_t)k - 1 - (uint32_t)(rel - left_len)))) & 3u;
				depth = md;
			} else {
				const uint32_t s = stage[p];
				code = s & 3u;
				depth = s >> 8;
			}
			wb |= (uint64_t)((0x54474341u >> (8 * code)) & 0xffu) << (8 * b);   // "ACGT"
			wd |= (uint64_t)depth << (8 * b);
		}
		if (n_bytes == 8) {
			*reinterpret_cast<uint64_t *>(bases + p0) = wb;
			*reinterpret_cast<uint64_t *>(depths + p0) = wd;
		} else {
			for (uint32_t b = 0; b < n_bytes; ++b) {
				bases[p0 + b] = (uint8_t)(wb >> (8 * b));
				depths[p0 + b] = (uint8_t)(wd >> (8 * b));
			}
		}
	}
}

} // namespace contigk
