// FILL: kernels of link_contig on the GPU (include/dbgk.h, FILL section; host side in dbgk_host_fill.h).
//
// A record (one line of a map_reads 2ctg file, or the two hits of one read) becomes the two directed entries of the LINK table
// (k_fill_orient writes them where k_link_orient would; sort, k_link_reduce and k_link_chain are reused as they are) and one
// entry of the gap statistics: the unordered contig pair and the gap the read leaves between its two alignments.  Two stable radix
// sorts (by gap, then by pair) put the records of one pair side by side, ascending by gap and in file order within a gap;
// k_fill_gapstat reduces every pair to the mode of its gaps.  The records of the mode are then one range of the sorted array:
// k_fill_consensus counts the bases of their slices column by column, k_fill_emit writes the scafftigs.
#pragma once
#include <stdint.h>

namespace fillk {

constexpr int kFillThreads = 256;
constexpr int kWave = 64;

struct Rec {                                   // == dbgk_fill_record
	int32_t read, read_len, align1_end, align2_start, contig1, contig2;
	uint8_t direct1, direct2, pad[2];
	int32_t reserved;
};
struct PairStat {                              // one contig pair: what decide_gap_size keeps, and where the records of its mode lie
	uint64_t key;                              // contig_lo << 32 | contig_hi
	int32_t mode, mode_freq, total_freq, variance;
	uint64_t mode_start;                       // position of the first record of the mode in the sorted array
};
struct GapDesc {                               // one gap of the layout with a mode > 0
	uint64_t span_start;                       // its spanning reads: sorted positions [span_start, span_start + n_span)
	uint64_t cons_off;                         // its columns in the consensus buffer
	uint32_t n_span;
	int32_t gap;
	int32_t left_contig, right_contig;
	uint32_t left_direct, right_direct;        // 'F' / 'R'
};
struct EmitItem {
	uint64_t src;                              // kind 0: first base in bases; 1: LAST base taken, read backwards; 2: first byte in cons
	uint32_t kind, pad;
};
struct Counters {
	unsigned long long pooled;                 // records in the gap statistics
	unsigned long long pairs;                  // slots handed out by k_fill_gapstat
};

constexpr int kStatusHostPath = 1;             // a slice held a byte other than A C G T N
constexpr int kStatusBadSlice = 2;             // a slice does not lie inside its read

// one thread per record.  FROM_HITS: the record is (hits[2 i], hits[2 i + 1]) of read first_read + i; reads map_reads would not
// have written to the 2ctg file (a hit unmapped, both on one contig: map_reads.cpp:59-73) leave dropped entries and count nowhere.
// parse_read_ends_map_file, link_func.cpp:175-217: FF, RR, FR, RF give ctg1 -> ctg3 and ctg4 -> ctg2, there is no gap filter.
template <bool FROM_HITS>
__global__ __launch_bounds__(kFillThreads) void k_fill_orient(const Rec *__restrict__ recs, const linkk::Hit *__restrict__ hits, uint64_t n,
                                                              uint32_t n_contigs, uint32_t first_read, uint64_t first_record,
                                                              uint64_t *__restrict__ keys, uint64_t *__restrict__ vals,
                                                              uint64_t *__restrict__ pair_keys, uint64_t *__restrict__ gap_keys,
                                                              uint64_t *__restrict__ gap_vals, int4 *__restrict__ rinfo,
                                                              linkk::Counters *ctr, Counters *fctr)
{
	__shared__ unsigned int s_cnt[7];
	if (threadIdx.x < 7) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	for (uint64_t i = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFillThreads) {
		int32_t read, a1e, a2s, c1, c2;
		uint32_t d1, d2;
		bool present = true;
		if (FROM_HITS) {
			const uint4 *p = reinterpret_cast<const uint4 *>(hits + 2 * i);
			const uint4 a0 = p[0], a1 = p[1], b0 = p[2], b1 = p[3];
			read = (int32_t)(first_read + (uint32_t)i);
			c1 = (int32_t)a0.x; a1e = (int32_t)a0.z; d1 = a1.w;
			c2 = (int32_t)b0.x; a2s = (int32_t)b0.y; d2 = b1.w;
			// (hits come from the device: their contig indices are checked here, those of records by the host)
			present = c1 != -1 && c2 != -1 && c1 != c2 && (uint32_t)c1 < n_contigs && (uint32_t)c2 < n_contigs;
		} else {
			const uint4 *p = reinterpret_cast<const uint4 *>(recs + i);
			const uint4 a = p[0], b = p[1];
			read = (int32_t)a.x; a1e = (int32_t)a.z; a2s = (int32_t)a.w; c1 = (int32_t)b.x; c2 = (int32_t)b.y;
			d1 = b.z & 0xff; d2 = (b.z >> 8) & 0xff;
		}
		const uint32_t gap = (uint32_t)a2s - (uint32_t)a1e - 1u;   // int arithmetic of the reference, wrapping
		uint64_t k0 = linkk::kDropped, k1 = linkk::kDropped, pk = linkk::kDropped;
		if (present) {
			const bool f1 = d1 == 'F', r1 = d1 == 'R', f2 = d2 == 'F', r2 = d2 == 'R';
			const int cls = (f1 && r2) ? 0 : (r1 && f2) ? 1 : (f1 && f2) ? 2 : (r1 && r2) ? 3 : 4;
			atomicAdd(&s_cnt[cls], 1u);
			if (cls != 4) {
				const uint32_t id1 = 2u * (uint32_t)c1 + 1, id2 = 2u * (uint32_t)c2 + 1;
				const uint32_t ctg1 = id1 + (r1 ? 1 : 0), ctg2 = id1 + (f1 ? 1 : 0), ctg3 = id2 + (r2 ? 1 : 0), ctg4 = id2 + (f2 ? 1 : 0);
				k0 = ((uint64_t)ctg1 << 32) | ctg3;
				k1 = ((uint64_t)ctg4 << 32) | ctg2;
				atomicAdd(&s_cnt[5], 1u);
			}
			const uint32_t lo = (uint32_t)(c1 < c2 ? c1 : c2), hi = (uint32_t)(c1 < c2 ? c2 : c1);
			pk = ((uint64_t)lo << 32) | hi;
			atomicAdd(&s_cnt[6], 1u);
		}
		const uint64_t r = first_record + i, e = 2 * r;
		*reinterpret_cast<ulonglong2 *>(keys + e) = make_ulonglong2(k0, k1);      // e is even: 16-byte aligned
		*reinterpret_cast<ulonglong2 *>(vals + e) = make_ulonglong2((e << 32) | gap, ((e + 1) << 32) | gap);
		pair_keys[r] = pk;
		gap_keys[r] = gap ^ 0x80000000u;                                          // ascending as signed ints
		gap_vals[r] = (r << 32) | gap;
		rinfo[r] = make_int4(read, a1e, c1, (int)d1);
	}
	__syncthreads();
	if (threadIdx.x < 5 && s_cnt[threadIdx.x]) atomicAdd(&ctr->cls[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
	if (threadIdx.x == 5 && s_cnt[5]) atomicAdd(&ctr->kept, (unsigned long long)s_cnt[5]);
	if (threadIdx.x == 6 && s_cnt[6]) atomicAdd(&fctr->pooled, (unsigned long long)s_cnt[6]);
}

// after the sort by gap: the key of the second sort is the pair of the record a value names
__global__ __launch_bounds__(kFillThreads) void k_fill_gather(const uint64_t *__restrict__ vals, const uint64_t *__restrict__ pair_keys,
                                                              uint64_t n, uint64_t *__restrict__ keys)
{
	for (uint64_t i = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFillThreads)
		keys[i] = pair_keys[vals[i] >> 32];
}

// first position in (from, end) whose element differs from that at `from`, in a range where equal elements lie side by side:
// gallop, then bisect.  SAME(j) says whether element j equals element from.
template <class Same>
__device__ __forceinline__ uint64_t fill_run_end(uint64_t from, uint64_t end, Same same)
{
	uint64_t lo = from, step = 1;                  // same(lo) holds
	uint64_t hi = end;                             // same(hi) does not hold (or hi == end)
	while (lo + step < end) {
		if (!same(lo + step)) { hi = lo + step; break; }
		lo += step;
		step *= 2;
	}
	while (hi - lo > 1) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (same(mid)) lo = mid; else hi = mid;
	}
	return hi;
}

// decide_gap_size (link_contig.cpp:569-610) over the sorted records: the thread of a pair's first record walks the runs of equal
// gaps of its pair (ascending, so on equal frequency the smallest gap stays: strict >), then sums |gap - mode| * freq in int
// arithmetic.  Run ends are found by galloping, so a run of thousands of records costs a few steps.
__global__ __launch_bounds__(kFillThreads) void k_fill_gapstat(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ vals,
                                                               uint64_t n, PairStat *__restrict__ out, Counters *fctr)
{
	for (uint64_t i = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFillThreads) {
		const uint64_t key = keys[i];
		if (i > 0 && keys[i - 1] == key) continue;
		const uint64_t end = fill_run_end(i, n, [&](uint64_t j) { return keys[j] == key; });
		int32_t mode = 0, mode_freq = 0;
		uint64_t mode_start = i;
		for (uint64_t j = i; j < end;) {
			const uint32_t g = (uint32_t)vals[j];
			const uint64_t e = fill_run_end(j, end, [&](uint64_t m) { return (uint32_t)vals[m] == g; });
			const int32_t freq = (int32_t)(e - j);
			if (freq > mode_freq) { mode = (int32_t)g; mode_freq = freq; mode_start = j; }
			j = e;
		}
		uint32_t var = 0;                          // int average_variance, wrapping
		for (uint64_t j = i; j < end;) {
			const uint32_t g = (uint32_t)vals[j];
			const uint64_t e = fill_run_end(j, end, [&](uint64_t m) { return (uint32_t)vals[m] == g; });
			const int32_t d = (int32_t)(g - (uint32_t)mode);
			var += (uint32_t)(d < 0 ? -d : d) * (uint32_t)(e - j);
			j = e;
		}
		const int32_t total = (int32_t)(end - i);
		PairStat s;
		s.key = key;
		s.mode = mode;
		s.mode_freq = mode_freq;
		s.total_freq = total;
		s.variance = (int32_t)var / total;
		s.mode_start = mode_start;
		out[atomicAdd(&fctr->pairs, 1ull)] = s;
	}
}

// the consensus of the filled gaps (fill_gaps_inside_scaffold, link_contig.cpp:465-509).  One wavefront takes 64 columns of one
// gap, a lane one column; the wave loops over the gap's spanning reads, so the 64 byte loads of one read are consecutive
// addresses, forward or backward.  The counts of A C G T N live in registers; a slice with any other byte sends the whole gap
// to the host's counted path (status 1), and the bytes written here are then not used.  Per column the byte with the highest
// count, the smallest byte value on a tie (ascending map<char,int>, strict >): A < C < G < N < T.  The count goes out per
// column; the support rate is a float sum in column order and is formed by the host.
// The spanning reads are first checked, 64 at a time: a slice outside its read (undefined in the reference) marks the gap
// (status 2) and none of its bytes is read.
__global__ __launch_bounds__(kFillThreads) void k_fill_consensus(const uint2 *__restrict__ work, uint64_t n_work, const GapDesc *__restrict__ gaps,
                                                                 const uint64_t *__restrict__ svals, const int4 *__restrict__ rinfo,
                                                                 const uint8_t *__restrict__ reads, const uint64_t *__restrict__ read_off,
                                                                 uint32_t n_reads, uint8_t *__restrict__ cons, uint32_t *__restrict__ cons_freq,
                                                                 int *__restrict__ status)
{
	const uint32_t lane = threadIdx.x & (kWave - 1);
	const uint64_t wave = ((uint64_t)blockIdx.x * kFillThreads + threadIdx.x) / kWave;
	const uint64_t n_waves = (uint64_t)gridDim.x * (kFillThreads / kWave);
	for (uint64_t w = wave; w < n_work; w += n_waves) {
		const uint2 unit = work[w];
		const GapDesc G = gaps[unit.x];
		const uint32_t col = unit.y * kWave + lane;
		const uint32_t gap = (uint32_t)G.gap;
		bool bad = false;
		for (uint32_t m = lane; m < G.n_span; m += kWave) {
			const int4 r = rinfo[svals[G.span_start + m] >> 32];
			if ((uint32_t)r.x >= n_reads || r.y < 0) bad = true;
			else if ((uint64_t)r.y + gap > read_off[r.x + 1] - read_off[r.x]) bad = true;
		}
		if (__any(bad)) {
			if (lane == 0) status[unit.x] = kStatusBadSlice;
			continue;
		}
		uint32_t nA = 0, nC = 0, nG = 0, nT = 0, nN = 0;
		bool other = false;
		for (uint32_t m0 = 0; m0 < G.n_span; m0 += kWave) {
			// lane l holds spanning read m0 + l of this round: where its slice begins and whether it is reverse-complemented
			uint64_t my_at = 0;
			uint32_t my_rc = 0;
			if (m0 + lane < G.n_span) {
				const int4 r = rinfo[svals[G.span_start + m0 + lane] >> 32];
				my_at = read_off[r.x] + (uint64_t)r.y;
				my_rc = (r.z == G.left_contig && (uint32_t)r.w != G.left_direct) || (r.z == G.right_contig && (uint32_t)r.w != G.right_direct);
			}
			const uint32_t rounds = G.n_span - m0 < (uint32_t)kWave ? G.n_span - m0 : (uint32_t)kWave;
			for (uint32_t l = 0; l < rounds; ++l) {
				const uint64_t at = __shfl(my_at, (int)l);
				const uint32_t rc = __shfl(my_rc, (int)l);
				if (col < gap) {
					uint32_t c = rc ? linkk::link_complement(reads[at + (gap - 1 - col)]) : reads[at + col];
					nA += c == 'A'; nC += c == 'C'; nG += c == 'G'; nT += c == 'T'; nN += c == 'N';
					other |= !(c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N');
				}
			}
		}
		if (col < gap) {
			uint32_t best = 'A', freq = nA;
			if (nC > freq) { best = 'C'; freq = nC; }
			if (nG > freq) { best = 'G'; freq = nG; }
			if (nN > freq) { best = 'N'; freq = nN; }
			if (nT > freq) { best = 'T'; freq = nT; }
			cons[G.cons_off + col] = (uint8_t)best;
			cons_freq[G.cons_off + col] = freq;
		}
		if (__any(other) && lane == 0) status[unit.x] = kStatusHostPath;
	}
}

// scafftig read-out: as k_link_emit, 8 output bytes per thread and bisection to the item of the first one.  An item is a run of
// bases read forward (a contig, possibly cut short), a run read backward and complemented (a reversed contig, possibly cut
// short: its first bases are the contig's last), or a run of consensus bytes.
__global__ __launch_bounds__(kFillThreads) void k_fill_emit(const uint8_t *__restrict__ bases, const uint8_t *__restrict__ cons,
                                                            const EmitItem *__restrict__ items, const uint64_t *__restrict__ item_off,
                                                            uint32_t n_items, uint64_t total, uint8_t *__restrict__ out)
{
	const uint64_t n_words = (total + 7) / 8;
	for (uint64_t w = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * kFillThreads) {
		const uint64_t p0 = w * 8;
		uint32_t lo = 0, hi = n_items;                 // the last item with item_off[t] <= p0 (empty items share an offset: take the last)
		while (hi - lo > 1) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (item_off[mid] <= p0) lo = mid; else hi = mid;
		}
		uint32_t t = lo;
		uint64_t t_begin = item_off[t], t_end = item_off[t + 1];
		EmitItem it = items[t];
		uint64_t word = 0;
		const uint32_t n_bytes = (uint32_t)(total - p0 < 8 ? total - p0 : 8);
		for (uint32_t b = 0; b < n_bytes; ++b) {
			const uint64_t p = p0 + b;
			while (p >= t_end) {                       // (p < total == item_off[n_items]: there is a later item that holds p)
				++t;
				t_begin = t_end;
				t_end = item_off[t + 1];
				it = items[t];
			}
			const uint64_t k = p - t_begin;
			uint32_t c;
			if (it.kind == 0) c = bases[it.src + k];
			else if (it.kind == 1) c = linkk::link_complement(bases[it.src - k]);
			else c = cons[it.src + k];
			word |= (uint64_t)c << (8 * b);
		}
		if (n_bytes == 8) {
			*reinterpret_cast<uint64_t *>(out + p0) = word;
		} else {
			for (uint32_t b = 0; b < n_bytes; ++b) out[p0 + b] = (uint8_t)(word >> (8 * b));
		}
	}
}

} // namespace fillk
