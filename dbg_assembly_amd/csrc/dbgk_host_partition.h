// dbgk_host_partition.h -- part of libdbgk.so's host side (one translation unit: included by dbgk.hip, in this order).
// PARTITION engine, host side: reset, geometry (plan_partition), record stores and kernel attributes (setup_partition)
#pragma once

static int reset_state(dbgk_handle *h)
{
	bool counters_done = false;
	// (direct-block form: the build writes every block of the table, also the empty ones -- nothing to zero)
	if (h->kfreq && !(h->part && h->kf_blocks)) HIPCHK(hipMemsetAsync(h->counts, 0, h->n_counts, h->stream));
	if (h->wide) {
		if (h->wpart) { // the region build overwrites every slot of the main table: zero it only if something writes it before
			h->wzero_pending = true;
			h->wbuilt = false;
			h->pending_kmers = 0;
			h->wgeom.pass = 0;
			h->wgeom.pass_j0 = 0;
			h->wpass_open = true;
			h->wplanned = false;
			h->wnext = 0;
			h->wpasses_done = 0;
			h->exchanged = false;
			HIPCHK(hipMemsetAsync(h->wstore.cnt1, 0, (size_t)h->wgeom.n_l1 * 4, h->stream));
			HIPCHK(hipMemsetAsync(h->wstore.ovf_n, 0, 16, h->stream));
			HIPCHK(hipMemsetAsync(h->wstore.outgoing_n, 0, 8, h->stream));
		} else {
			HIPCHK(hipMemsetAsync(h->wnodes, 0, h->tslots * sizeof(WNode), h->stream));
		}
		HIPCHK(hipMemsetAsync(h->wside, 0, kWideSideSlots * sizeof(WNode), h->stream));
	} else if (h->kfreq && !h->part) {
	} else if (h->part) {
		// the region build of finalize overwrites every slot, so the 16 B/slot memset is only needed
		// if a direct-path write (merge) happens first
		h->zero_pending = true;
		h->incr = false;
		int rc = clear_record_store(h, true); // (one launch: the stores' control arrays and the counters)
		if (rc) return rc;
		counters_done = true;
	} else {
		int rc = zero_table_now(h);
		if (rc) return rc;
	}
	if (h->track) HIPCHK(hipMemsetAsync(h->first_pos, 0xFF, h->tslots * 8, h->stream));
	h->pos_base = 0;
	if (!counters_done) {
		HIPCHK(hipMemsetAsync(h->d_ctr, 0, sizeof(Counters), h->stream));
		HIPCHK(hipMemsetAsync(&h->d_ctr->polyA_slot, 0xFF, sizeof(unsigned long long), h->stream));
	}
	h->finalized = false;
	h->total_reads = 0;
	h->host_other_bytes = 0;
	return DBGK_OK;
}

// Decide whether the PARTITION engine is used, and the geometry of its record stores: host arithmetic on the configuration, the
// hash modulus `size` and whether the handle counts k-mers (KFREQ, and there in direct blocks).  Nothing of a handle is read or written.
//   geometry: level-1 bucket = slot >> r, r >= 20 chosen so that n1 = ceil(size / 2^r) <= 1024;
//   final bucket = slot >> 12 (one 4096-slot region); n2 = 2^(r-12) sub-buckets per level-1 bucket.
//   An 8-byte record must hold q = hash / size, r slot bits and 6 neighbour bits.
static int plan_partition(const dbgk_config &cfg, uint64_t size, bool kfreq, bool kf_blocks, PartPlan &plan)
{
	plan = PartPlan();
	memset(&plan.geom, 0, sizeof plan.geom);
	plan.tslots = size;
	const ModMagic magic = make_mod_magic(size);
	if (kfreq && kf_blocks) { // direct blocks: `size` = 4^k, slot = the key with its block index permuted (kf_slot_of_key)
		PartGeom &G = plan.geom;
		const uint32_t bits = 2u * (uint32_t)cfg.kmer_size; // >= 26
		// level-1 bucket = slot >> r: 256 buckets where the table allows (the wave-per-bucket level-1 kernel), level 2 then
		// splits a bucket into its 2^(r - 16) <= 1024 blocks in one pass
		const uint32_t r = std::max(20u, std::min(26u, bits - 8u));
		G.size = size;
		G.magic = magic;
		if (size < (1ull << 32)) G.div = make_div32_magic((uint32_t)size);
		G.r = r;
		G.n1 = (uint32_t)(size >> r);
		G.n2 = 1u << (r - kKfBlockBits);
		G.n_final = (uint32_t)(size >> kKfBlockBits);
		G.n_ranks = 1;
		G.rank = 0;
		G.B = G.n1;
		G.n_sub = kSubStores;
		G.b_lo = 0;
		G.nb_own = G.n1;
		G.slot_lo = 0;
		G.slot_hi = size;
		G.n_regions_own = G.n_final;
		const double per_slot = (double)cfg.expected_kmers / (double)size;
		// a level-1 bucket sums 2^(r - 16) blocks of very different weight (canonical k-mers favour small key values): more slack
		// than the hashed form's 5 %; a single block may hold 2.2 times the average
		G.cap1 = (uint64_t)(per_slot * (double)(1ull << r) * 1.2 / (double)G.n_sub) + 65536 / G.n_sub + 8192;
		G.cap2 = ((uint64_t)(per_slot * (double)(1ull << kKfBlockBits) * 2.6) + 1024 + 3) & ~3ull; // (16-bit records, read four at a time)
		G.r_rec = r;
		G.l2_shift = kKfBlockBits - (uint32_t)kRegionBits; // level 2 splits by block, not by 4096-slot region
		G.kf = 2u;
		G.l2_records = 16u * (uint32_t)l2_threads((int)G.n2);
		G.kf_mask = (uint32_t)((1ull << (bits - kKfBlockBits)) - 1ull);
		if (G.n1 > (uint32_t)kL1MaxB || G.n2 > (uint32_t)kMaxBuckets) return DBGK_OK; // (cannot happen for 13 <= k <= 18)
		plan.shard_rank = 0;
		plan.part = true;
		plan.three = false;
		return DBGK_OK;
	}
	const uint32_t n_ranks = cfg.shard_count > 1 ? cfg.shard_count : 1;
	const int want = cfg.engine == DBGK_ENGINE_SEEDIDX ? DBGK_ENGINE_DIRECT // the seed index uses the plain table
	                 : cfg.engine == DBGK_ENGINE_KFREQ ? DBGK_ENGINE_AUTO   // KFREQ: only if the geometry is feasible
	                                                      : cfg.engine;
	const bool want_shard = cfg.shard_count >= 1; // shard_count == 1: one-rank sharded handle (same protocol, for testing)
	if (want_shard && cfg.shard_index >= n_ranks) return DBGK_ERR_ARG;
	if (!want_shard) {
		if (want == DBGK_ENGINE_DIRECT) return DBGK_OK;
		if (want == DBGK_ENGINE_AUTO && cfg.expected_kmers == 0) return DBGK_OK; // streaming use: total unknown
	}
	uint32_t r = 22; // measured on cfg2 (round 2, profiles/r02_r_sweep.txt): r = 20 / 21 / 22 -> 17.3 / 16.5 / 16.3 ms per step
	if (const char *e = DBGK_EXPERIMENT_ENV("DBGK_PART_R")) r = (uint32_t)std::max(20, std::min(24, atoi(e))); // tuning knob: level-1 bucket = slot >> r
	while (((size + (1ull << r) - 1) >> r) > (uint64_t)kL1MaxB) r++;
	const uint64_t qmax = ~0ull / size;
	int qbits = 0;
	while (qbits < 64 && (qmax >> qbits)) qbits++;
	while (r > 20 && qbits + (int)r + 6 > 64 && ((size + (1ull << (r - 1)) - 1) >> (r - 1)) <= (uint64_t)kL1MaxB) r--; // small tables: q needs the bits
	// level 1 fans out to <= 1024 buckets, level 2 to 2^(r-12) <= 4096 final buckets per level-1 bucket: 2^34 slots
	const bool feasible = (1u << (r - kRegionBits)) <= (uint32_t)kMaxBucketsL2 && (qbits + (int)r + 6) <= 64 && size >= (1ull << 26) &&
	                      size < (1ull << 34);
	if (!feasible || (want_shard && want == DBGK_ENGINE_DIRECT)) {
		if (want == DBGK_ENGINE_PARTITION || want_shard) {
			g_last_error = "PARTITION engine (and any sharded handle) needs 2^26 <= table_slots < 2^34";
			return DBGK_ERR_ARG;
		}
		return DBGK_OK;
	}
	for (uint64_t x : {0ull, 1ull, 0x0123456789ABCDEFull, ~0ull, 488296166657017542ull}) {
		if (hash_code_inverse(hash_code(x)) != x) {
			g_last_error = "hash_code_inverse self-check failed";
			return DBGK_ERR_STATE;
		}
	}
	PartGeom &G = plan.geom;
	G.size = size;
	G.magic = magic;
	if (size < (1ull << 32)) G.div = make_div32_magic((uint32_t)size);
	G.r = r;
	G.n1 = (uint32_t)((size + (1ull << r) - 1) >> r);
	G.n2 = 1u << (r - kRegionBits);
	G.n_final = (uint32_t)((size + kRegionSlots - 1) >> kRegionBits);
	G.n_ranks = n_ranks;
	G.rank = want_shard ? cfg.shard_index : 0;
	plan.shard_rank = G.rank;
	G.B = (G.n1 + n_ranks - 1) / n_ranks;
	G.n_sub = kSubStores;
	G.b_lo = std::min(G.rank * G.B, G.n1);
	G.nb_own = std::min(G.B, G.n1 - G.b_lo);
	G.slot_lo = (uint64_t)G.b_lo << r;
	G.slot_hi = std::min<uint64_t>(size, ((uint64_t)G.b_lo + G.nb_own) << r);
	G.n_regions_own = (uint32_t)((G.slot_hi - G.slot_lo + kRegionSlots - 1) >> kRegionBits);
	if (G.nb_own == 0 || (uint64_t)n_ranks * G.B * G.n_sub > (uint64_t)kMaxInboxEntries) {
		g_last_error = "shard_count too large for this table size";
		return DBGK_ERR_ARG;
	}
	// expected_kmers = occurrences THIS handle extracts; a region receives the global density
	const uint64_t expected = cfg.expected_kmers ? cfg.expected_kmers : size * 2 / n_ranks;
	const double per_slot = (double)expected / (double)size;
	G.cap1 = (uint64_t)(per_slot * (double)(1ull << r) * 1.05 / (double)G.n_sub) + 65536 / G.n_sub + (G.n_sub > 1 ? 8192 : 0); // per sub-store
	G.cap2 = (uint64_t)(per_slot * (double)n_ranks * (double)kRegionSlots * 1.15) + 512;
	// every bucket starts on a 128-byte line (the 16-byte record loads of level 2 and of the build are aligned), and a bucket is an ODD
	// number of lines long: the append points of neighbouring buckets then fall on neighbouring lines modulo any power of two, whatever
	// the memory system's channel interleave (on one box WIDE level 2 moved between 44 and 50 ms from process to process until its strides
	// were odd; other boxes run it at 44 or at 49 whatever the strides, profiles/r05_cfg5_wide_l2_variants.txt)
	G.cap1 = ((G.cap1 + 15u) & ~15ull) | 16u;
	G.cap2 = ((G.cap2 + 15u) & ~15ull) | 16u;
	G.r_rec = r;
	G.l2_shift = 0;
	G.l2_records = 16u * (uint32_t)l2_threads((int)G.n2);
	plan.tslots = G.slot_hi - G.slot_lo;
	plan.sharded = want_shard;
	plan.part = true;
	static const bool no_three = DBGK_EXPERIMENT_ENV("DBGK_THREE_LEVEL") && atoi(DBGK_EXPERIMENT_ENV("DBGK_THREE_LEVEL")) == 0; // measurements
	// measured with cfg2's 1.2 G records, level 2 alone: n2 = 4096 (8.6 G slots) 17.6 ms in one pass, 9.7 ms in two;
	// n2 = 2048 (5 G slots) 6.9 ms in one pass, 9.5 in two -- so only the 4096-way fan-out is split
	plan.three = G.n2 > 2048u && !no_three;
	if (plan.three) {
		plan.fan_mid = G.n2 / 64u; // 64
		uint32_t lg = 0;
		while ((1u << lg) < plan.fan_mid) lg++;
		const uint64_t cap_mid = ((uint64_t)(per_slot * (double)n_ranks * (double)(1ull << (r - lg)) * 1.08) + 8192 + 15u) & ~15ull;
		plan.g_mid = G;
		plan.g_mid.n2 = plan.fan_mid;
		plan.g_mid.l2_records = 16u * (uint32_t)l2_threads((int)plan.fan_mid);
		plan.g_mid.l2_shift = 6;      // the low 6 bits of the final-bucket index are left to the final pass
		plan.g_mid.cap2 = cap_mid;
		plan.g_fin = G;
		plan.g_fin.n_ranks = 1;       // its input is this handle's own mid store
		plan.g_fin.rank = 0;
		plan.g_fin.n_sub = 1;
		plan.g_fin.r = r - lg;
		plan.g_fin.n1 = G.n1 * plan.fan_mid;
		plan.g_fin.B = G.nb_own * plan.fan_mid;
		plan.g_fin.b_lo = G.b_lo * plan.fan_mid;
		plan.g_fin.nb_own = G.nb_own * plan.fan_mid;
		plan.g_fin.n2 = 64;
		plan.g_fin.l2_records = 16u * (uint32_t)l2_threads(64);
		plan.g_fin.cap1 = cap_mid;
	}
	return DBGK_OK;
}

static void apply_plan(dbgk_handle *h, const PartPlan &plan)
{
	h->part = plan.part;
	h->sharded = plan.sharded;
	h->three = plan.three;
	h->fan_mid = plan.fan_mid;
	h->tslots = plan.tslots;
	h->shard_rank = plan.shard_rank;
	h->geom = plan.geom;
	h->g_mid = plan.g_mid;
	h->g_fin = plan.g_fin;
}

// allocate the record stores of the PARTITION engine (geometry already planned)
static int l1_register_lds(bool wide); // dbgk_host_level1.h: the dynamic LDS sizes of the level-1 launch tables

static int setup_partition(dbgk_handle *h)
{
	if (!h->part) return DBGK_OK;
	const PartGeom &G = h->geom;
	PartStore &P = h->store;
	memset(&P, 0, sizeof P);
	const uint64_t expected = h->cfg.expected_kmers ? h->cfg.expected_kmers : h->size * 2 / G.n_ranks;
	// records that find their bucket full are kept as {key, lb, rb} triples and inserted through the global
	// path after the build: a key that occurs more often than a final bucket holds (cap2, ~1.15x the mean
	// bucket fill) sends its surplus here, so this bounds the share of occurrences that may belong to such
	// heavy hitters (high-copy repeats): 1/16 of the input + 1 M; beyond it finalize returns DBGK_ERR_CAPACITY
	P.ovf_cap = expected / 16 + (1ull << 20);
	P.spill_cap = (uint64_t)G.n_regions_own * 8 + (1ull << 16);
	P.outgoing_cap = 1ull << 16;
	const size_t n_entries = (size_t)G.n_ranks * G.B * G.n_sub;
	const size_t l1_bytes = n_entries * G.cap1 * 8, l2_bytes = (size_t)G.nb_own * G.n2 * G.cap2 * (G.kf == 2u ? 2 : 8); // (direct blocks: 16-bit records)
	// (+ 64 bytes: level 2 and the build load their records in pairs, and the second half of a bucket's last pair may lie behind the bucket)
	PartBufs &O = h->pbuf;
	bool ok = !O.l1.reserve(l1_bytes + 64) && !O.l2.reserve(l2_bytes + 64) && !O.cnt1.reserve(n_entries * 4) && !O.cnt2.reserve((size_t)G.nb_own * G.n2 * 4) &&
	          !O.ovf.reserve(P.ovf_cap * sizeof(Node)) && !O.spill.reserve(P.spill_cap * sizeof(Node)) && !O.ovf_n.reserve(16) &&
	          !O.tile_prefix.reserve((n_entries + 1) * 4) &&
	          !O.region_cursor.reserve(((size_t)kMaxBuildLaunches + 2 + G.n_regions_own) * sizeof(unsigned int)) && // + redo cursor, count, list
	          !O.outgoing.reserve(P.outgoing_cap * sizeof(Node)) && !O.outgoing_n.reserve(8);
	if (ok && h->sharded) ok = !O.inbox.reserve(l1_bytes + 64) && !O.inbox_cnt.reserve(n_entries * 4);
	if (!ok) {
		g_last_error = "hipMalloc of the PARTITION record stores failed";
		return DBGK_ERR_NOMEM;
	}
	// side table for the surplus of heavy hitters; on a sharded handle it may hold keys of any shard and is
	// offered to every rank after the build (dbgk_shard_heavy), like the overflow list
	if (O.hh.reserve(kHeavyHitterSlots * sizeof(Node))) return DBGK_ERR_NOMEM;
	P.l1 = O.l1;
	P.l2 = O.l2;
	P.cnt1 = O.cnt1;
	P.cnt2 = O.cnt2;
	P.ovf = O.ovf;
	P.spill = O.spill;
	P.ovf_n = O.ovf_n;
	P.outgoing = O.outgoing;
	P.outgoing_n = O.outgoing_n;
	P.hh = O.hh;
	HIPCHK(hipMemsetAsync(P.hh, 0, kHeavyHitterSlots * sizeof(Node), h->stream)); // once: afterwards it is zeroed again only when it was used (clear_record_store)
	P.hh_size = kHeavyHitterSlots;
	P.hh_magic = make_mod_magic(kHeavyHitterSlots);
	P.inbox = h->sharded ? O.inbox.p : O.l1.p;
	P.inbox_cnt = h->sharded ? O.inbox_cnt.p : O.cnt1.p;
	// EARLY level 2 (early_l2): a handle that extracts into its own inbox scatters what earlier batches stored while the next
	// batch is on the link.  Not for shards (their inbox is filled by the exchange), the three-level form, 32-bit KFREQ records
	const bool no_early = dbgk_hook("early_l2") && atoi(dbgk_hook("early_l2")) == 0; // (read per handle: measurements, and the tests compare the two)
	P.l2_done = P.l2_upto = nullptr;
	if (!h->sharded && !h->three && G.kf != 2u && !no_early) {
		if (h->pbuf.l2_done.reserve(2 * n_entries * 4)) return DBGK_ERR_NOMEM; // done[] and upto[]
		HIPCHK(hipMemsetAsync(h->pbuf.l2_done, 0, 2 * n_entries * 4, h->stream));
		P.l2_done = h->pbuf.l2_done;
		P.l2_upto = h->pbuf.l2_done + n_entries;
	}
	h->l2_seen_kmers = 0;
	h->store_capacity = expected;
	if (h->three) {
		const size_t n_mid = (size_t)G.nb_own * h->fan_mid;
		if (h->pbuf.mid.reserve(n_mid * h->g_mid.cap2 * 8 + 64) || h->pbuf.cnt_mid.reserve(n_mid * 4) || h->pbuf.tile_prefix2.reserve((n_mid + 1) * 4)) {
			g_last_error = "hipMalloc of the mid-level record store failed";
			return DBGK_ERR_NOMEM;
		}
		h->s_mid = P;           // reads the inbox like level 2, writes the mid store
		h->s_mid.l2 = h->pbuf.mid;
		h->s_mid.cnt2 = h->pbuf.cnt_mid;
		h->s_fin = P;           // reads the mid store, writes the final buckets where level 2 would
		h->s_fin.inbox = h->pbuf.mid;
		h->s_fin.inbox_cnt = h->pbuf.cnt_mid;
	}
	int rc = l1_register_lds(false); // every level-1 form of dbgk_l1_form.h's lists
	if (rc) return rc;
#ifdef DBGK_EXPERIMENTS // timing experiments (DBGK_DEBUG_MODE, results are wrong): not in the product library
	DBGK_LDS_ATTR((k_scatter_l2<1>), sizeof(ScatterLdsL2));
	DBGK_LDS_ATTR((k_scatter_l2<2>), sizeof(ScatterLdsL2));
	DBGK_LDS_ATTR((k_scatter_l2<3>), sizeof(ScatterLdsL2));
#endif
	DBGK_LDS_ATTR((k_scatter_l2<0>), sizeof(ScatterLdsL2));
	DBGK_LDS_ATTR((k_scatter_l2<0, kMaxBuckets, true>), sizeof(ScatterLdsL2));
	DBGK_LDS_ATTR((k_scatter_l2<0, 2048>), sizeof(ScatterLdsL2T<2048>));
	DBGK_LDS_ATTR((k_scatter_l2<0, 4096>), sizeof(ScatterLdsL2T<4096>));
#define DBGK_BUILD_ATTR(...) DBGK_LDS_ATTR((k_build_regions<__VA_ARGS__>), sizeof(BuildLds))
	DBGK_BUILD_ATTR(0, false, false, false); DBGK_BUILD_ATTR(0, true, false, false); DBGK_BUILD_ATTR(0, false, true, false); DBGK_BUILD_ATTR(0, true, true, false);
	DBGK_BUILD_ATTR(0, false, false, true);  DBGK_BUILD_ATTR(0, true, false, true);  DBGK_BUILD_ATTR(0, false, true, true);  DBGK_BUILD_ATTR(0, true, true, true);
	DBGK_BUILD_ATTR(0, false, false, false, true); DBGK_BUILD_ATTR(0, true, false, false, true); DBGK_BUILD_ATTR(0, false, true, false, true);
	DBGK_BUILD_ATTR(0, true, true, false, true);
#ifdef DBGK_EXPERIMENTS
	DBGK_BUILD_ATTR(1, false, false, false); DBGK_BUILD_ATTR(2, false, false, false); DBGK_BUILD_ATTR(3, false, false, false);
	DBGK_BUILD_ATTR(1, false, false, true);  DBGK_BUILD_ATTR(2, false, false, true);  DBGK_BUILD_ATTR(3, false, false, true);
#endif
#undef DBGK_BUILD_ATTR
	DBGK_LDS_ATTR((k_kf_build_blocks<false, true>), sizeof(KfBlockLds));
	DBGK_LDS_ATTR((k_kf_build_blocks<true, true>), sizeof(KfBlockLds));
	DBGK_LDS_ATTR((k_kf_build_blocks<false, false>), sizeof(KfBlockLds));
	DBGK_LDS_ATTR((k_kf_build_blocks<true, false>), sizeof(KfBlockLds));
	DBGK_LDS_ATTR((k_kf_build_blocks<false, false, true>), sizeof(KfBlockLds));
	DBGK_LDS_ATTR((k_kf_build_blocks<true, false, true>), sizeof(KfBlockLds));
	return DBGK_OK;
}

static int ensure_slot(dbgk_handle *h, StageSlot &s);
