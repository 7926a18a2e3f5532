// LINK: kernels of link_scaffold on the GPU (include/dbgk.h, LINK section; host side in dbgk_host_link.h).
//
// A record (one line of a map_pair 2ctg file, or the first hits of the two mates of a pair) becomes two directed entries
// (ctg1 -> ctg3, ctg4 -> ctg2; link_scaffold/link_func.cpp:262-321, :367-423).  Entry 2r and 2r + 1 of record r keep that place in one
// array over all batches, so an entry's index IS its place in the reference's record order.  The entries are sorted by
// (source, target) with a stable radix sort; k_link_reduce turns every run of equal keys into one link (count and gap sum of its
// first 1023 entries, add_data_into_link :458-463, and the index of its first entry); a second sort by (source, first index) puts a
// node's links into the order the reference's list has them in, and k_link_chain writes them out.
#pragma once
#include <stdint.h>

namespace linkk {

constexpr int kLinkThreads = 256;
constexpr uint32_t kFreqCap = 1023;            // CtgLink.freq is 10 bits (link_func.h:34)
constexpr uint64_t kDropped = ~0ull;           // key of an entry that is not kept: sorts behind every real key

struct Pair {                                  // == dbgk_link_pair
	int32_t contig1, start1, end1, contig2, start2, end2;
	uint8_t direct1, direct2, pad[2];
	int32_t reserved;
};
struct Hit {                                   // == dbgk_map_hit
	int32_t contig, read_start, read_end, contig_start, contig_end, mismatches, align_len, direct;
};
struct Entry {                                 // == dbgk_link_entry
	uint32_t target, freq;
	int64_t size;
};
struct Item {                                  // == dbgk_link_item
	int32_t contig, value;
};
struct Counters {
	unsigned long long cls[5];                 // FR, RF, FF, RR, wrong
	unsigned long long kept;                   // records that passed the gap filter
	unsigned long long links;                  // slots handed out by k_link_reduce
};

// the two directed entries of one record.  Node of contig c is 2c + 1, its reverse strand 2c + 2; all arithmetic is the reference's
// 32-bit int arithmetic.  cls: 0 FR, 1 RF, 2 FF, 3 RR, 4 wrong.
__device__ __forceinline__ void link_orient(int mate_pair, int32_t insert, const uint32_t *__restrict__ lens, int32_t c1, int32_t s1,
                                            int32_t e1, uint32_t d1, int32_t c2, int32_t s2, int32_t e2, uint32_t d2, int &cls, uint32_t &ctg1,
                                            uint32_t &ctg2, uint32_t &ctg3, uint32_t &ctg4, int32_t &gap)
{
	const bool f1 = d1 == 'F', r1 = d1 == 'R', f2 = d2 == 'F', r2 = d2 == 'R';
	cls = (f1 && r2) ? 0 : (r1 && f2) ? 1 : (f1 && f2) ? 2 : (r1 && r2) ? 3 : 4;
	const uint32_t id1 = 2u * (uint32_t)c1 + 1, id2 = 2u * (uint32_t)c2 + 1;
	const uint32_t l1 = lens[c1], l2 = lens[c2], I = (uint32_t)insert;
	uint32_t g = 0;
	ctg1 = ctg2 = ctg3 = ctg4 = 0;
	// the class that reads  mate 1 forward on the left contig, mate 2 reverse on the right one  is FR for pair ends and RF for mate
	// pairs, and so on: -m 1 swaps FR with RF and FF with RR (link_func.cpp:366)
	const int shape = cls == 4 ? 4 : (mate_pair ? (cls ^ 1) : cls);
	switch (shape) {
		case 0: ctg1 = id1; ctg2 = id1 + 1; ctg3 = id2; ctg4 = id2 + 1; g = I - (l1 - (uint32_t)s1) - (uint32_t)e2; break;                    // :262-273, :378-388
		case 1: ctg1 = id2; ctg2 = id2 + 1; ctg3 = id1; ctg4 = id1 + 1; g = I - (l2 - (uint32_t)s2) - (uint32_t)e1; break;                    // :274-285, :367-377
		case 2: ctg1 = id1; ctg2 = id1 + 1; ctg4 = id2; ctg3 = id2 + 1; g = I - (l1 - (uint32_t)s1) - (l2 - (uint32_t)s2); break;             // :286-297, :401-411
		case 3: ctg2 = id1; ctg1 = id1 + 1; ctg3 = id2; ctg4 = id2 + 1; g = I - (l1 - (l1 - (uint32_t)e1)) - (uint32_t)e2; break;             // :298-309, :389-400
		default: break;
	}
	gap = (int32_t)g;
}

// one thread per record.  FROM_HITS: the record is the pair (hits1[i], hits2[i]); pairs map_pair would not have written to the 2ctg
// file (a mate unmapped, or both on one contig: map_pair.cpp:315-323) leave two dropped entries and count nowhere.
template <bool FROM_HITS>
__global__ __launch_bounds__(kLinkThreads) void k_link_orient(const Pair *__restrict__ pairs, const Hit *__restrict__ hits1,
                                                              const Hit *__restrict__ hits2, uint64_t n, const uint32_t *__restrict__ lens,
                                                              uint32_t n_contigs, int mate_pair, int32_t insert, uint64_t first_entry,
                                                              uint64_t *__restrict__ keys, uint64_t *__restrict__ vals, Counters *ctr)
{
	__shared__ unsigned int s_cnt[6];
	if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	for (uint64_t i = (uint64_t)blockIdx.x * kLinkThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kLinkThreads) {
		int32_t c1, s1, e1, c2, s2, e2;
		uint32_t d1, d2;
		bool present = true;
		if (FROM_HITS) {
			const uint4 *p1 = reinterpret_cast<const uint4 *>(hits1 + i), *p2 = reinterpret_cast<const uint4 *>(hits2 + i);
			const uint4 a0 = p1[0], a1 = p1[1], b0 = p2[0], b1 = p2[1];
			c1 = (int32_t)a0.x; s1 = (int32_t)a0.w; e1 = (int32_t)a1.x; d1 = a1.w;
			c2 = (int32_t)b0.x; s2 = (int32_t)b0.w; e2 = (int32_t)b1.x; d2 = b1.w;
			present = c1 != -1 && c2 != -1 && c1 != c2;
		} else {
			const uint4 *p = reinterpret_cast<const uint4 *>(pairs + i);
			const uint4 a = p[0], b = p[1];
			c1 = (int32_t)a.x; s1 = (int32_t)a.y; e1 = (int32_t)a.z; c2 = (int32_t)a.w; s2 = (int32_t)b.x; e2 = (int32_t)b.y;
			d1 = b.z & 0xff; d2 = (b.z >> 8) & 0xff;
		}
		// (the host has checked the contig indices of a pair batch; hits come from the device, so they are checked here)
		if (present && ((uint32_t)c1 >= n_contigs || (uint32_t)c2 >= n_contigs)) present = false;
		uint64_t k0 = kDropped, k1 = kDropped;
		int32_t gap = 0;
		if (present) {
			int cls;
			uint32_t ctg1, ctg2, ctg3, ctg4;
			link_orient(mate_pair, insert, lens, c1, s1, e1, d1, c2, s2, e2, d2, cls, ctg1, ctg2, ctg3, ctg4, gap);
			atomicAdd(&s_cnt[cls], 1u);
			// if (gap_size > -InsertSize / 2 && gap_size <= InsertSize), :317 / :419
			if (cls != 4 && gap > -(insert / 2) && gap <= insert) {
				k0 = ((uint64_t)ctg1 << 32) | ctg3;
				k1 = ((uint64_t)ctg4 << 32) | ctg2;
				atomicAdd(&s_cnt[5], 1u);
			}
		}
		const uint64_t e = first_entry + 2 * i;
		// value: the entry's index (its place in record order) above its gap
		const ulonglong2 kk = make_ulonglong2(k0, k1);
		const ulonglong2 vv = make_ulonglong2((e << 32) | (uint32_t)gap, ((e + 1) << 32) | (uint32_t)gap);
		*reinterpret_cast<ulonglong2 *>(keys + e) = kk;      // e is even: 16-byte aligned
		*reinterpret_cast<ulonglong2 *>(vals + e) = vv;
	}
	__syncthreads();
	if (threadIdx.x < 5 && s_cnt[threadIdx.x]) atomicAdd(&ctr->cls[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
	if (threadIdx.x == 5 && s_cnt[5]) atomicAdd(&ctr->kept, (unsigned long long)s_cnt[5]);
}

// the capped segmented reduce over the sorted entries: the thread of a run's first entry walks the run, at most 1023 entries of
// it (the entries behind are never counted, :459), and hands the link a slot.  The sort is stable, so the first entry of a run is
// the one with the smallest index.  Slots come in no particular order; k_link_chain orders them.
__global__ __launch_bounds__(kLinkThreads) void k_link_reduce(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ vals,
                                                              uint64_t n, uint64_t *__restrict__ order_keys, uint64_t *__restrict__ order_vals,
                                                              Entry *__restrict__ slots, Counters *ctr)
{
	for (uint64_t i = (uint64_t)blockIdx.x * kLinkThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kLinkThreads) {
		const uint64_t key = keys[i];
		if (key == kDropped || (i > 0 && keys[i - 1] == key)) continue;
		const uint64_t v0 = vals[i];
		int64_t size = (int32_t)(uint32_t)v0;
		uint32_t freq = 1;
		for (uint64_t j = i + 1; j < n && freq < kFreqCap && keys[j] == key; ++j) {
			size += (int32_t)(uint32_t)vals[j];
			++freq;
		}
		const unsigned long long slot = atomicAdd(&ctr->links, 1ull);
		Entry e;
		e.target = (uint32_t)key;
		e.freq = freq;
		e.size = size;
		slots[slot] = e;
		order_keys[slot] = (key & 0xffffffff00000000ull) | (v0 >> 32);   // (source, index of the first entry)
		order_vals[slot] = slot;
	}
}

// links in chain order: sorted position j takes the slot order_vals[j]; its source goes to src[j]
__global__ __launch_bounds__(kLinkThreads) void k_link_chain(const uint64_t *__restrict__ order_keys, const uint64_t *__restrict__ order_vals,
                                                             uint64_t n, const Entry *__restrict__ slots, Entry *__restrict__ out,
                                                             uint32_t *__restrict__ src)
{
	for (uint64_t j = (uint64_t)blockIdx.x * kLinkThreads + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kLinkThreads) {
		const uint4 e = *reinterpret_cast<const uint4 *>(slots + order_vals[j]);
		*reinterpret_cast<uint4 *>(out + j) = e;
		src[j] = (uint32_t)(order_keys[j] >> 32);
	}
}

// reverse_complement of the reference (seqKmer.cpp:72-81): N and n are kept, A C G T in either case give the upper-case
// complement, every other byte gives N
__device__ __forceinline__ uint32_t link_complement(uint32_t c)
{
	const uint32_t u = c & 0xdf;
	return (c == 'N' || c == 'n') ? c : u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N';
}

// scaffold read-out: the items lie back to back in the output, item t at out[item_off[t], item_off[t + 1]).  One thread writes 8
// consecutive output bytes with one store: it finds the item of its first byte by bisection and moves on to the next items as it
// crosses their ends (items of one base are common).  contig >= 0: value 0 copies the contig, value 1 writes its reverse
// complement; contig < 0: a run of N.
__global__ __launch_bounds__(kLinkThreads) void k_link_emit(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ ctg_off,
                                                            const Item *__restrict__ items, const uint64_t *__restrict__ item_off,
                                                            uint32_t n_items, uint64_t total, uint8_t *__restrict__ out)
{
	const uint64_t n_words = (total + 7) / 8;
	for (uint64_t w = (uint64_t)blockIdx.x * kLinkThreads + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * kLinkThreads) {
		const uint64_t p0 = w * 8;
		uint32_t lo = 0, hi = n_items;                 // the last item with item_off[t] <= p0 (empty items share an offset: take the last)
		while (hi - lo > 1) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (item_off[mid] <= p0) lo = mid; else hi = mid;
		}
		uint32_t t = lo;
		uint64_t t_begin = item_off[t], t_end = item_off[t + 1];
		Item it = items[t];
		uint64_t c_begin = it.contig >= 0 ? ctg_off[it.contig] : 0;
		uint64_t word = 0;
		const uint32_t n_bytes = (uint32_t)(total - p0 < 8 ? total - p0 : 8);
		for (uint32_t b = 0; b < n_bytes; ++b) {
			const uint64_t p = p0 + b;
			while (p >= t_end) {                       // (p < total == item_off[n_items]: there is a later item that holds p)
				++t;
				t_begin = t_end;
				t_end = item_off[t + 1];
				it = items[t];
				c_begin = it.contig >= 0 ? ctg_off[it.contig] : 0;
			}
			uint32_t c;
			if (it.contig < 0) c = 'N';
			else if (it.value == 0) c = bases[c_begin + (p - t_begin)];
			else c = link_complement(bases[c_begin + (t_end - 1 - p)]);
			word |= (uint64_t)c << (8 * b);
		}
		if (n_bytes == 8) {
			*reinterpret_cast<uint64_t *>(out + p0) = word;
		} else {
			for (uint32_t b = 0; b < n_bytes; ++b) out[p0 + b] = (uint8_t)(word >> (8 * b));
		}
	}
}

} // namespace linkk
