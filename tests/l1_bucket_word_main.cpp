// Stand-alone host program for tests/test_l1_bucket_word_cpu.py: the bucket word of the pipelined level-1 forms
// (l1_bucket_word_pack / l1_bucket_word_unpack, dbg_assembly_amd/csrc/dbgk_partition.h) and the LDS layout it rests on, on the CPU.
//   l1_bucket_word_main layout        "layout hist_words= lbase_dist= rank_bits= head_off= head_bytes= uniform_stage= uniform_bytes=
//                                      prefix_head_off= prefix_stage= prefix_bytes= max_b= threads="
//   l1_bucket_word_main word REC      REC = 8 or 4, the record size.  The LDS address of every histogram entry of either histogram (dummy
//                                     bins included) with every rank a tile can give (0 .. 16 * threads - 1 records, in bytes), the two maxima
//                                     together among them; then every value of the entry field with the edge ranks and every value of
//                                     the rank field with the edge entries.  Per pair: unpack(pack) gives the pair back, the word of a
//                                     larger entry is larger whatever the ranks (the "has no bucket" test compares whole words), and
//                                     the staged address lbase + rank is the one the (bucket << 16 | rank) encoding gives.
//                                     Prints "word rec= checked= bad=".
// Built by the test with the HIP compiler as the other host programs of the suite, host side under ASan + UBSan.
#define DBGK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dbgk.h"
#include "dbgk_env.h"
#include "dbgk_kernels.h"
#include "dbgk_partition.h"

using namespace dbgk;

static uint64_t g_checked = 0, g_bad = 0;
static const uint32_t kHead = (uint32_t)offsetof(UniformPipeLds, s); // where the histogram area lies in the kernels' LDS

// one (entry, rank) pair: the round trip, and the staged address against today's other encoding
static void check_pair(uint32_t entry, uint32_t rank_bytes, uint32_t rec)
{
	const uint32_t w = l1_bucket_word_pack(entry, rank_bytes);
	uint32_t e = ~0u, r = ~0u;
	l1_bucket_word_unpack(w, e, r);
	g_checked++;
	if (e != entry || r != rank_bytes) g_bad++;
	// an entry of the histogram area: histogram h, bucket b.  lbase holds stage + 8 * (first staged index); with the plain encoding the
	// record goes to stage[first + rank].  first: any value a scan can give, here derived from the pair itself.
	if (entry % 4u == 0u && entry >= kHead && entry < kHead + 2u * kL1HistWords * 4u && rank_bytes % rec == 0u && rank_bytes / rec < 16u * (uint32_t)kL1Threads) {
		const uint32_t stage = (uint32_t)offsetof(PrefixPipeLds, stage);
		const uint32_t b = ((entry - kHead) / 4u) % kL1HistWords, rank = rank_bytes / rec;
		const uint32_t first = (b * 2654435761u) % (16u * (uint32_t)kL1Threads - rank); // first + rank < 16 * threads
		const uint32_t plain_word = (b << 16) | rank;
		const uint32_t want = stage + rec * (first + (plain_word & 0xFFFFu));
		const uint32_t lbase_bytes = stage + rec * first;
		if (lbase_bytes + r != want || (plain_word >> 16) != b) g_bad++;
		if (e + kL1LbaseDist < kHead + (uint32_t)offsetof(L1PipeLds, lbase) || e + kL1LbaseDist + 4u > kHead + (uint32_t)sizeof(L1PipeLds) + 64u * 4u) g_bad++; // (the last 64 are the second histogram's dummy bins: never read)
	}
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "layout")) {
		printf("layout hist_words=%u lbase_dist=%u rank_bits=%u head_off=%zu head_bytes=%zu uniform_stage=%zu uniform_bytes=%zu prefix_head_off=%zu prefix_stage=%zu "
		       "prefix_bytes=%zu max_b=%d threads=%d\n",
		       kL1HistWords, kL1LbaseDist, kL1RankBits, offsetof(UniformPipeLds, s), sizeof(L1PipeLds), offsetof(UniformPipeLds, stage), sizeof(UniformPipeLds),
		       offsetof(PrefixPipeLds, s), offsetof(PrefixPipeLds, stage), sizeof(PrefixPipeLds), kL1MaxB, kL1Threads);
		return 0;
	}
	if (argc >= 3 && !strcmp(argv[1], "word")) {
		const uint32_t rec = (uint32_t)atoi(argv[2]);
		if (rec != 8u && rec != 4u) return 2;
		const uint32_t max_rank = rec * (16u * (uint32_t)kL1Threads - 1u), max_entry = kHead + 2u * kL1HistWords * 4u - 4u;
		const uint32_t entry_field = 1u << (32u - kL1RankBits), rank_field = 1u << kL1RankBits;
		if (max_rank >= rank_field || max_entry >= entry_field) g_bad++;
		// every entry x every rank of a tile
		for (uint32_t entry = kHead; entry <= max_entry; entry += 4u)
			for (uint32_t rank = 0; rank <= max_rank; rank += rec) check_pair(entry, rank, rec);
		check_pair(max_entry, max_rank, rec); // (the maxima together, said once more by name)
		// the whole width of either field against the other's edges
		const uint32_t edge_ranks[] = {0u, rec, max_rank - rec, max_rank, rank_field - 1u};
		const uint32_t edge_entries[] = {0u, kHead, kHead + (uint32_t)kL1MaxB * 4u - 4u, kHead + (uint32_t)kL1MaxB * 4u, kHead + kL1HistWords * 4u - 4u, kHead + kL1HistWords * 4u,
		                                 kHead + (kL1HistWords + (uint32_t)kL1MaxB) * 4u - 4u, kHead + (kL1HistWords + (uint32_t)kL1MaxB) * 4u, max_entry, entry_field - 1u};
		for (uint32_t entry = 0; entry < entry_field; entry++)
			for (uint32_t rank : edge_ranks) check_pair(entry, rank, rec);
		for (uint32_t rank = 0; rank < rank_field; rank++)
			for (uint32_t entry : edge_entries) check_pair(entry, rank, rec);
		// whole words compare like their entries: a dummy bin's word is never below the first word without a bucket
		for (uint32_t h = 0; h < 2u; h++) {
			const uint32_t no_bucket = l1_bucket_word_pack(kHead + (h * kL1HistWords + (uint32_t)kL1MaxB) * 4u, 0u);
			for (uint32_t b = 0; b < kL1HistWords; b++)
				for (uint32_t rank : {0u, rec, max_rank}) {
					const uint32_t w = l1_bucket_word_pack(kHead + (h * kL1HistWords + b) * 4u, rank);
					g_checked++;
					if ((w < no_bucket) != (b < (uint32_t)kL1MaxB)) g_bad++;
				}
		}
		printf("word rec=%u checked=%" PRIu64 " bad=%" PRIu64 "\n", rec, g_checked, g_bad);
		return g_bad ? 1 : 0;
	}
	return 2;
}
