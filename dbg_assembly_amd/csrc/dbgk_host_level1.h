// dbgk_host_level1.h -- part of libdbgk.so's host side (one translation unit: included by dbgk.hip, in this order).
// one batch on the device: which level-1 / insert kernel form a batch takes (launch_batch) and its pre-passes
#pragma once

#include "dbgk_l1_form.h"

// the decision (dbgk_l1_form.h) sees the kernels' tile geometry through this
constexpr L1Limits kL1Limits{(uint32_t)kL1Threads, (uint32_t)kPkWords, kPrefixMaxW, kPrefixPipeMaxB, (uint32_t)kWL1Threads, kWPkWords, kWPipePkWords};
static_assert(DBGK_L1_THREADS != 1024 || DBGK_L1_MAXB != 1024 || kL1Limits == L1Limits{}, "dbgk_l1_form.h: the defaults of L1Limits are the product build's geometry");

// The launch tables: a row per instantiation of dbgk_l1_form.h's lists -- the form, the kernel, its dynamic LDS bytes.
template <class Fn>
struct L1Row {
	L1Form form;
	Fn fn;
	uint32_t lds;
};
template <int DBG, int WIDE_D, int C, bool RAGGED, bool LIN, bool REG, bool PACKED, bool FULL, bool K17>
constexpr uint32_t uniform_lds()
{
	return LIN ? sizeof(UniformLdsLin<LIN ? C : 8>) : uniform_pipelined(DBG, WIDE_D, RAGGED, LIN, REG, K17) ? sizeof(UniformPipeLds) : sizeof(UniformLds);
}
template <int WIDE_D, int C, bool K17>
constexpr uint32_t prefix_lds() { return K17 ? sizeof(PrefixPipeLds) : sizeof(PrefixLds); }
#define DBGK_ROW(...) {l1_uniform(__VA_ARGS__), &k_extract_scatter_uniform<__VA_ARGS__>, uniform_lds<__VA_ARGS__>()},
static const L1Row<decltype(&k_extract_scatter_uniform<>)> kL1UniformRows[] = {DBGK_L1_UNIFORM_ROWS(DBGK_ROW)};
#undef DBGK_ROW
#define DBGK_ROW(...) {l1_prefix(__VA_ARGS__), &k_extract_scatter_prefix<__VA_ARGS__>, prefix_lds<__VA_ARGS__>()},
static const L1Row<decltype(&k_extract_scatter_prefix<>)> kL1PrefixRows[] = {DBGK_L1_PREFIX_ROWS(DBGK_ROW)};
#undef DBGK_ROW
#define DBGK_ROW(...) {l1_flat(__VA_ARGS__), &k_extract_scatter<__VA_ARGS__>, sizeof(ScatterLds)},
static const L1Row<decltype(&k_extract_scatter<false>)> kL1FlatRows[] = {DBGK_L1_FLAT_ROWS(DBGK_ROW)};
#undef DBGK_ROW
#define DBGK_ROW(...) {l1_flat_lin(__VA_ARGS__), &k_extract_scatter_lin<__VA_ARGS__>, sizeof(ScatterLdsLin<8>)},
static const L1Row<decltype(&k_extract_scatter_lin<false>)> kL1FlatLinRows[] = {DBGK_L1_FLAT_LIN_ROWS(DBGK_ROW)};
#undef DBGK_ROW
#define DBGK_ROW(...) {l1_wide_flat(__VA_ARGS__), &k_wide_scatter_l1<__VA_ARGS__>, sizeof(WL1Lds)},
static const L1Row<decltype(&k_wide_scatter_l1<false, 0>)> kL1WideFlatRows[] = {DBGK_L1_WIDE_FLAT_ROWS(DBGK_ROW)};
#undef DBGK_ROW
#define DBGK_ROW(WD, PIPE) {l1_wide_uniform(WD, PIPE), &k_wide_scatter_l1_uniform<WD, PIPE>, PIPE ? sizeof(WL1PipeLds) : sizeof(WL1Lds)},
static const L1Row<decltype(&k_wide_scatter_l1_uniform<0>)> kL1WideUniformRows[] = {DBGK_L1_WIDE_UNIFORM_ROWS(DBGK_ROW)};
#undef DBGK_ROW

// kernels with more than 64 KiB of dynamic LDS have to say so: every row of the tables
template <class Fn, size_t N>
static int l1_set_lds_attrs(const L1Row<Fn> (&rows)[N])
{
	for (const L1Row<Fn> &r : rows)
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(r.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds));
	return DBGK_OK;
}
static int l1_register_lds(bool wide)
{
	int rc;
	if (wide) return (rc = l1_set_lds_attrs(kL1WideFlatRows)) ? rc : l1_set_lds_attrs(kL1WideUniformRows);
	if ((rc = l1_set_lds_attrs(kL1UniformRows)) || (rc = l1_set_lds_attrs(kL1PrefixRows)) || (rc = l1_set_lds_attrs(kL1FlatRows))) return rc;
	return l1_set_lds_attrs(kL1FlatLinRows);
}

// launch the row of `form` with that row's LDS size; a form without a row is an error, never another kernel
template <class Fn, size_t N, class... Args>
static int l1_launch(const L1Row<Fn> (&rows)[N], const L1Form &form, uint64_t grid, int threads, hipStream_t stream, Args... args)
{
	for (const L1Row<Fn> &r : rows)
		if (r.form == form) {
			hipLaunchKernelGGL(r.fn, dim3((uint32_t)grid), dim3(threads), r.lds, stream, args...);
			return DBGK_OK;
		}
	char text[192];
	l1_form_text(form, text, sizeof text);
	g_last_error = std::string("no level-1 kernel for the form ") + text;
	return DBGK_ERR_ARG;
}

// the handle's part of the facts, the hooks and the experiment switches: read once per batch
static L1Facts l1_facts(const dbgk_handle *h, bool wrec)
{
	L1Facts f;
	f.lim = kL1Limits;
	f.part = h->part; f.seed = h->seed; f.kfreq = h->kfreq; f.wide = h->wide; f.wrec = wrec;
	f.kmer_size = h->cfg.kmer_size;
	f.max_read_len = (uint64_t)h->cfg.max_read_len;
	f.n1 = h->geom.n1; f.kf = h->geom.kf; f.geom_size = h->geom.size; f.size = h->size;
	auto hook_int = [](const char *name) { const char *v = dbgk_hook(name); return v ? atoi(v) : -1; };
	f.l1_linear = hook_int("l1_linear");
	f.l1_prefix = hook_int("l1_prefix");
	f.l1_plain = dbgk_hook("l1_plain") != nullptr;
	f.wide_l1_plain = dbgk_hook("wide_l1_plain") != nullptr;
	f.l1_flat = DBGK_EXPERIMENT_ENV("DBGK_L1_FLAT") != nullptr;
	const char *dbg = DBGK_EXPERIMENT_ENV("DBGK_DEBUG_MODE"), *lin_c = DBGK_EXPERIMENT_ENV("DBGK_L1_LINEAR_C");
	f.dbg_set = dbg != nullptr;
	f.dbg_mode = dbg ? atoi(dbg) : 0;
	f.no_reg = DBGK_EXPERIMENT_ENV("DBGK_L1_NO_REG") != nullptr;
	f.lin_c = lin_c ? (atoi(lin_c) == 12 ? 12 : 8) : 0;
	return f;
}

// scratch of the prefix form for a batch of n_reads reads / n_bases bases (grown as needed; the stream is idle when it grows)
static int ensure_prefix_scratch(dbgk_handle *h, uint64_t n_reads, uint64_t n_bases, bool need_packed)
{
	const uint64_t tiles = (n_bases / 15 + n_reads) / kL1Threads + 2; // a read of W windows has at most W / 15 + 1 lanes
	const uint64_t cr = std::max(n_reads, h->cap_reads), ct = std::max(tiles, (h->cap_bases / 15 + h->cap_reads) / kL1Threads + 2);
	if (cr * sizeof(ReadLanes) > h->pf_ent.cap || ct * sizeof(PrefixTile) > h->pf_tiles.cap) {
		HIPCHK(hipStreamSynchronize(h->stream));
		const uint64_t blocks = (cr + kPrefixBlock * kPrefixItems - 1) / (kPrefixBlock * kPrefixItems) + 1;
		if (h->pf_ent.reserve(cr * sizeof(ReadLanes)) || h->pf_tile_first.reserve((ct + 1) * 4) || h->pf_tiles.reserve(ct * sizeof(PrefixTile)) ||
		    h->pf_bsum.reserve(blocks * 8))
			return DBGK_ERR_NOMEM;
	}
	if (h->pf_tot.reserve(sizeof(PrefixTotals))) return DBGK_ERR_NOMEM;
	const uint64_t words = (n_bases + 15) / 16 + 16;
	if (need_packed && words * 4 > h->pf_packed.cap) {
		HIPCHK(hipStreamSynchronize(h->stream));
		if (h->pf_packed.reserve(words * 4, (h->cap_bases / 16 + 16) * 4)) return DBGK_ERR_NOMEM;
	}
	return DBGK_OK;
}

static int early_l2(dbgk_handle *h);

// the lane prefix of a batch for the prefix form: three short kernels over the offsets, then the tiles' descriptors
template <int CC>
static void launch_prefix_passes(dbgk_handle *h, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases)
{
	const uint32_t n_blocks = (uint32_t)((n_reads + kPrefixBlock * kPrefixItems - 1) / (kPrefixBlock * kPrefixItems));
	const uint32_t tiles_max = (uint32_t)std::min<uint64_t>((n_bases / 15 + n_reads) / kL1Threads + 1, h->pf_tiles.cap / sizeof(PrefixTile));
	const uint32_t k = (uint32_t)h->cfg.kmer_size, max_len = (uint32_t)h->cfg.max_read_len;
	hipLaunchKernelGGL((k_prefix_count<CC>), dim3(n_blocks), dim3(kPrefixBlock), 0, h->stream, d_offsets, n_reads, k, max_len, h->pf_bsum);
	hipLaunchKernelGGL(k_prefix_blocks, dim3(1), dim3(kPrefixBlock), 0, h->stream, h->pf_bsum, n_blocks, h->pf_tot);
	hipLaunchKernelGGL((k_prefix_emit<CC>), dim3(n_blocks), dim3(kPrefixBlock), 0, h->stream, d_offsets, n_reads, k, max_len, h->pf_bsum, h->pf_ent,
	                   h->pf_tile_first, h->d_ctr);
	hipLaunchKernelGGL((k_prefix_tiles<CC>), dim3((tiles_max + 255) / 256), dim3(256), 0, h->stream, h->pf_ent, h->pf_tile_first, h->pf_tot, k, n_bases,
	                   h->pf_tiles);
}

// level 1 of the record engines: the launches of the batch's plan, each through its family's table
static int launch_l1(dbgk_handle *h, const L1Plan &plan, const ReadBatch &rb, const uint64_t *d_offsets, uint64_t n_reads)
{
	for (int i = 0; i < plan.n; i++) {
		const L1Launch &l = plan.launch[i];
		const L1Geom &g = l.geom;
		const bool wide = l.form.family == L1Family::WideFlat || l.form.family == L1Family::WideUniform;
		const uint64_t wgs = (uint64_t)h->n_cu * (wide ? 1 : l1_wgs_per_cu()); // 140 KiB of LDS and more: one workgroup per CU
		const uint64_t grid = l.tiles ? std::min(l.tiles, wgs) : wgs;
		int rc = DBGK_ERR_ARG;
		switch (l.form.family) {
		case L1Family::Uniform: {
			if (g.n_lanes >> 32) { // (the kernels count tiles in 32 bits; uniform_mode never plans such a launch)
				g_last_error = "level 1: a launch of 2^32 lanes or more";
				return DBGK_ERR_ARG;
			}
			ReadBatch r = rb;
			if (l.n_reads != n_reads) { // regular tiles / the reads behind them: equal lengths, the launch's own reads
				if (r.packed) r.packed += l.first_read * g.L / 16; // (a whole number of words: a tile is a multiple of 16 bases)
				else r.bases += l.first_read * g.L;
				r.n_bases = l.n_reads * g.L;
			}
			rc = l1_launch(kL1UniformRows, l.form, grid, kL1Threads, h->stream, r, UniformGeom{g.L, g.W, g.Q, g.qmagic, g.n_lanes, g.lq, g.tile_blocks},
			               d_offsets, h->geom, h->store, h->d_ctr.p);
			break;
		}
		case L1Family::Prefix:
			rc = l1_launch(kL1PrefixRows, l.form, grid, kL1Threads, h->stream, rb, h->pf_ent.p, h->pf_tiles.p, h->pf_tot.p, h->geom, h->store, h->d_ctr.p);
			break;
		case L1Family::Flat:
			rc = l1_launch(kL1FlatRows, l.form, grid, kL1Threads, h->stream, rb, h->geom, h->store, h->d_ctr.p);
			break;
		case L1Family::FlatLin:
			rc = l1_launch(kL1FlatLinRows, l.form, grid, kL1Threads, h->stream, rb, h->geom, h->store, h->d_ctr.p);
			break;
		case L1Family::WideFlat:
			rc = l1_launch(kL1WideFlatRows, l.form, grid, kWL1Threads, h->stream, rb, h->wgeom, h->wstore, h->wref(), h->d_ctr.p);
			break;
		case L1Family::WideUniform:
			rc = l1_launch(kL1WideUniformRows, l.form, grid, kWL1Threads, h->stream, rb, WUniformGeom{g.L, g.W, g.Q, g.qmagic, g.n_lanes}, h->wgeom,
			               h->wstore, h->wref(), h->d_ctr.p);
			break;
		}
		if (rc) return rc;
		if (h->l1_forms_total < dbgk_handle::kL1FormLog) h->l1_forms[h->l1_forms_total] = l.form; // what dbgk_l1_forms_text reports
		h->l1_forms_total++;
	}
	return DBGK_OK;
}

static int launch_batch(dbgk_handle *h, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                        uint64_t n_bases, uint32_t *d_start, uint32_t *d_dead, int has_long /* 0,1 or -1 = ask device */,
                        int64_t uniform_len = -1 /* every read this long; 0 = lengths differ; -1 = ask device */,
                        uint64_t len_max = 0 /* longest read of the batch (with uniform_len >= 0) */,
                        const uint32_t *d_packed = nullptr /* the batch as 2-bit codes instead of d_bases (then null) */)
{
	if (n_reads == 0) return DBGK_OK;
	if (h->seed && d_packed) return DBGK_ERR_ARG; // the seed index cuts its windows at 'N', which two bits cannot say
	if (h->seed) has_long = 1; // the dead bitmap carries the 'N' positions
	const uint64_t words = bitmap_words(n_bases);
	TimedSpan sp;
	int rc = early_l2(h); // level 2 of what the batches before this one stored: queued IN FRONT of this batch's level 1, i.e. it runs while
	if (rc) return rc;    // this batch is still on the link (the level-1 launch below waits for the copy, the level-2 round does not)
	rc = span_begin(h, PH_MARK, sp);
	if (rc) return rc;
	static_assert(offsetof(Counters, len_max) + sizeof(unsigned long long) - offsetof(Counters, any_dead) == 20, "per-batch fields are contiguous");
	if (d_offsets) HIPCHK(hipMemsetAsync(&h->d_ctr->any_dead, 0, 20, h->stream)); // any_dead, len_min_inv, len_max: what k_mark reports per batch
	// The read-boundary bitmaps are what the general kernels navigate by; the PARTITION engine's level-1 kernel for
	// (nearly) equal-length reads does without them, so for such a batch only the statistics are taken.  A device
	// batch tells its shape only after those statistics: the bitmaps follow in a second pass if they are needed.
	auto mark_bits = [&](int with_stats) -> int {
		HIPCHK(hipMemsetAsync(d_start, 0, words * 4, h->stream));
		if (has_long != 0) HIPCHK(hipMemsetAsync(d_dead, 0, words * 4, h->stream));
		hipLaunchKernelGGL(k_mark, dim3(grid_for(h, n_reads)), dim3(kBlock), 0, h->stream, d_offsets, n_reads, n_bases,
		                   h->cfg.kmer_size, h->cfg.max_read_len, d_start, has_long != 0 ? d_dead : nullptr, h->d_ctr, with_stats);
		return DBGK_OK;
	};
	const bool wrec = h->wide && h->wpart && !h->wbuilt; // WIDE handle that is still collecting records
	L1Facts facts = l1_facts(h, wrec);
	facts.n_reads = n_reads;
	facts.n_bases = n_bases;
	facts.packed = d_packed != nullptr;
	L1Plan plan{};
	int umode = -1; // not decided yet
	bool use_prefix = false; // the prefix form (prefix_wanted) instead of the flat or the ragged one
	auto decide = [&]() { // (the batch's shape is known)
		facts.has_long = has_long;
		facts.uniform_len = uniform_len;
		facts.len_max = len_max;
		plan = l1_plan(facts);
		umode = plan.umode;
		use_prefix = plan.prefix;
	};
	// A batch of equal-length reads that came WITHOUT offsets (dbgk_push_reads_packed_uniform*): the equal-length level-1 forms of the
	// PARTITION / WIDE record engines never look at offsets -- the totals are added by a one-thread kernel and nothing else runs in
	// front of level 1; any other consumer gets the offsets made on the device first.
	const bool no_offsets = d_offsets == nullptr;
	auto make_offsets = [&]() -> int {
		if ((n_reads + 1) * 8 > h->uni_offsets.cap) {
			HIPCHK(hipStreamSynchronize(h->stream));
			if (h->uni_offsets.reserve((n_reads + 1) * 8, (h->cap_reads + 1) * 8)) return DBGK_ERR_NOMEM;
		}
		hipLaunchKernelGGL(k_iota_offsets, dim3(grid_for(h, n_reads + 1)), dim3(kBlock), 0, h->stream, h->uni_offsets, n_reads, (uint64_t)uniform_len);
		HIPCHK(hipMemsetAsync(&h->d_ctr->any_dead, 0, 20, h->stream));
		d_offsets = h->uni_offsets;
		return DBGK_OK;
	};
	const bool may_skip_bits = (h->part && !h->seed) || wrec;
	if (may_skip_bits && has_long >= 0 && uniform_len >= 0) decide();
	if (no_offsets && umode == 1) { // (umode 1 = equal lengths, nothing trimmed: every read has uniform_len - k + 1 windows)
		const unsigned long long w = uniform_len >= h->cfg.kmer_size ? (unsigned long long)(uniform_len - h->cfg.kmer_size + 1) * n_reads : 0ull;
		hipLaunchKernelGGL(k_add_totals, dim3(1), dim3(64), 0, h->stream, h->d_ctr, w, w);
	} else {
		if (no_offsets) {
			rc = make_offsets();
			if (rc) return rc;
		}
		if (may_skip_bits && (umode != 0 || use_prefix)) {
			hipLaunchKernelGGL(k_mark, dim3(grid_for(h, n_reads)), dim3(kBlock), 0, h->stream, d_offsets, n_reads, n_bases, h->cfg.kmer_size,
			                   h->cfg.max_read_len, (uint32_t *)nullptr, (uint32_t *)nullptr, h->d_ctr, 1); // statistics only
		} else {
			rc = mark_bits(1);
			if (rc) return rc;
		}
	}
	if (h->seed && n_bases)
		hipLaunchKernelGGL(k_mark_n, dim3(grid_for(h, (n_bases + 31) >> 5)), dim3(kBlock), 0, h->stream, d_bases, n_bases, d_dead);
	HIPCHK(hipGetLastError());
	if (has_long < 0 || (uniform_len < 0 && (h->part || wrec))) {
		HIPCHK(hipMemcpyAsync(&h->h_ctr->any_dead, &h->d_ctr->any_dead, 20, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
		if (has_long < 0) has_long = h->h_ctr->any_dead ? 1 : 0;
		if (uniform_len < 0) {
			uniform_len = ~h->h_ctr->len_min_inv == h->h_ctr->len_max ? (int64_t)h->h_ctr->len_max : 0;
			len_max = h->h_ctr->len_max;
		}
	}
	if (may_skip_bits && umode < 0) {
		decide();
		if (umode == 0 && !use_prefix) { // the general kernel after all: it needs the bitmaps
			rc = mark_bits(0);
			if (rc) return rc;
			HIPCHK(hipGetLastError());
		}
	}
	rc = span_end(h, sp);
	if (rc) return rc;
	const uint64_t id_base = h->total_reads; // contig index of the batch's first sequence (SEEDIDX)
	h->total_reads += n_reads;
	if (n_bases == 0) return DBGK_OK;

	ReadBatch rb{d_bases, n_bases, d_start, has_long ? d_dead : nullptr, h->cfg.kmer_size, d_packed, &h->d_ctr->other_seen};
	const uint64_t n_chunks = (n_bases + 15) >> 4;
	rc = span_begin(h, PH_INSERT, sp);
	if (rc) return rc;
	if (h->seed) {
		hipLaunchKernelGGL(k_seed_insert, dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, d_offsets, n_reads, id_base, h->tref(), h->d_ctr);
	} else if (wrec) {
		if (umode > 0) h->uniform_launches++;
		rc = launch_l1(h, plan, rb, d_offsets, n_reads);
		if (rc) return rc;
	} else if (h->wide) {
		rc = wide_ensure_zero(h);
		if (rc) return rc;
		if (has_long)
			hipLaunchKernelGGL(k_wide_extract_insert<true>, dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, h->wref(), h->d_ctr);
		else
			hipLaunchKernelGGL(k_wide_extract_insert<false>, dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, h->wref(), h->d_ctr);
	} else if (h->kfreq && !h->part) {
		if (has_long)
			hipLaunchKernelGGL(k_extract_count<true>, dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, reinterpret_cast<uint32_t *>(h->counts.p));
		else
			hipLaunchKernelGGL(k_extract_count<false>, dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, reinterpret_cast<uint32_t *>(h->counts.p));
	} else if (h->part) {
		if (use_prefix) {
			// lane prefix of the batch (three short kernels over the offsets), the batch itself as 2-bit words, then level 1
			h->prefix_launches++;
			rc = ensure_prefix_scratch(h, n_reads, n_bases, d_packed == nullptr);
			if (rc) return rc;
			if (!d_packed) {
				hipLaunchKernelGGL(k_pack_bases, dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, d_bases, n_bases, h->pf_packed, h->d_ctr);
				rb.packed = h->pf_packed;
			}
			if (plan.launch[0].form.c == 15) launch_prefix_passes<15>(h, d_offsets, n_reads, n_bases);
			else launch_prefix_passes<16>(h, d_offsets, n_reads, n_bases);
		} else if (umode > 0)
			h->uniform_launches++;
		rc = launch_l1(h, plan, rb, d_offsets, n_reads);
		if (rc) return rc;
	} else if (h->track) {
		if (has_long)
			hipLaunchKernelGGL((k_extract_insert<true, true>), dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, h->tref(), h->d_ctr,
			                   h->first_pos, h->pos_base);
		else
			hipLaunchKernelGGL((k_extract_insert<false, true>), dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, h->tref(), h->d_ctr,
			                   h->first_pos, h->pos_base);
		h->pos_base += n_bases;
	} else if (has_long) {
		hipLaunchKernelGGL((k_extract_insert<true, false>), dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, h->tref(), h->d_ctr,
		                   (unsigned long long *)nullptr, (uint64_t)0);
	} else {
		hipLaunchKernelGGL((k_extract_insert<false, false>), dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, rb, h->tref(), h->d_ctr,
		                   (unsigned long long *)nullptr, (uint64_t)0);
	}
	// bytes outside ACGTNacgtn were read as 'A'; if a kernel met one (Counters::other_seen) this batch's are counted now --
	// every workgroup of the launch leaves at once otherwise.  A packed batch has none: its packer counted them.
	if (!d_packed) hipLaunchKernelGGL(k_count_other_bytes, dim3(grid_for(h, n_chunks)), dim3(kBlock), 0, h->stream, d_bases, n_bases, h->d_ctr);
	HIPCHK(hipGetLastError());
	return span_end(h, sp);
}
