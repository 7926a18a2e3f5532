// CLEAN: host side of clean_adapter / clean_lowqual on the GPU (include/dbgk.h, CLEAN section; kernels in dbgk_clean.h)

struct dbgk_clean : StageDev {
	// the adapter set: codes back to back (padded to whole dwords), offsets[n + 1]
	DevBuf<uint8_t> d_ad;
	DevBuf<uint32_t> d_ad_off;
	uint64_t n_adapters = 0, adapter_bytes = 0;
	int32_t score_cutoff = 0;
	bool adapters_set = false;
	// Qual2Err of clean_lowqual.cpp:220-222 for the shift it was last built for
	DevBuf<double> d_table;
	int32_t table_shift = -1;
	// batch buffers, grown on demand
	DevBuf<uint8_t> d_seq, d_qual;
	DevBuf<uint64_t> d_off;
	DevBuf<uint8_t> d_out; // cleank::AdapterHit or cleank::LowqualBlock per read (both 24 bytes)
	DevBuf<uint32_t> d_long;
	DevBuf<cleank::CleanCounters> d_ctr;
	uint64_t cap_bytes = 0, cap_qual = 0, cap_reads = 0;
	StageEvents<4> ev;
	dbgk_clean_stats last{};
	// output stage (dbgk_host_emit.h): the batch whose offsets and records d_off / d_out hold, and its compact form
	bool have_batch = false;      // the last batch call succeeded: batch_n reads of b_seq / b_qual are resident
	uint64_t batch_n = 0;
	int32_t batch_kind = 0;       // DBGK_CLEAN_KIND_*: what d_out holds
	int32_t batch_shift = 0;      // the quality shift of a lowqual batch
	const uint8_t *b_seq = nullptr, *b_qual = nullptr; // d_seq / d_qual, or the caller's planes of a _device call; b_qual null: no quality plane
	EmitStage emit;
};

static_assert(sizeof(dbgk_adapter_hit) == 24 && sizeof(cleank::AdapterHit) == 24, "dbgk_adapter_hit is six int32");
static_assert(sizeof(dbgk_lowqual_block) == 24 && sizeof(cleank::LowqualBlock) == 24, "dbgk_lowqual_block layout");
static_assert(offsetof(dbgk_lowqual_block, start) == 8 && offsetof(dbgk_lowqual_block, trimmed) == 16, "dbgk_lowqual_block layout");

extern "C" int dbgk_clean_create(int device, dbgk_clean **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (device < 0) return DBGK_ERR_ARG;
	dbgk_clean *c = new (std::nothrow) dbgk_clean;
	if (!c) return DBGK_ERR_NOMEM;
	int rc = stage_open(*c, device);
	if (!rc) rc = c->ev.create();
	if (!rc) rc = emit_create(c->emit, emitk::CleanRule<DBGK_CLEAN_KIND_LOWQUAL>::kCounters, false); // (both kinds count the same seven)
	if (!rc && (c->d_ctr.reserve(sizeof(cleank::CleanCounters)) || c->d_table.reserve(256 * sizeof(double)))) rc = DBGK_ERR_NOMEM;
	if (rc) {
		dbgk_clean_destroy(c);
		return rc;
	}
	*out = c;
	return DBGK_OK;
}

extern "C" int dbgk_clean_destroy(dbgk_clean *c)
{
	if (!c) return DBGK_ERR_ARG;
	stage_drain(c->device, c->stream);
	emit_destroy(c->emit);
	delete c;
	return DBGK_OK;
}

extern "C" int dbgk_clean_set_adapters(dbgk_clean *c, const char *bases, const uint64_t *offsets, uint64_t n, int32_t score_cutoff)
{
	// a cutoff below 1 makes the reference report coordinates it never set (clean_adapter.cpp:115,129,193)
	if (!c || !offsets || offsets[0] != 0 || score_cutoff < 1 || n >= (1ull << 20)) return DBGK_ERR_ARG;
	for (uint64_t i = 0; i < n; ++i)
		if (offsets[i + 1] < offsets[i]) return DBGK_ERR_ARG;
	const uint64_t total = offsets[n];
	if ((total && !bases) || total >= (1ull << 29)) return DBGK_ERR_ARG; // read_len + adapter_len stays well inside int32
	std::vector<uint8_t> codes(((total + 3) & ~3ull) + 16, (uint8_t)cleank::kAdapterOther);
	for (uint64_t i = 0; i < total; ++i) {
		const uint32_t code = cleank::clean_code((uint8_t)bases[i]);
		codes[i] = (uint8_t)(code == cleank::kReadOther ? cleank::kAdapterOther : code);
	}
	std::vector<uint32_t> off32(n + 1);
	for (uint64_t i = 0; i <= n; ++i) off32[i] = (uint32_t)offsets[i];
	HIPCHK(hipSetDevice(c->device));
	c->adapters_set = false;
	c->d_ad.release(); c->d_ad_off.release();
	if (c->d_ad.reserve(codes.size()) || c->d_ad_off.reserve(off32.size() * 4)) return DBGK_ERR_NOMEM;
	HIPCHK(hipMemcpyAsync(c->d_ad, codes.data(), codes.size(), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->d_ad_off, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->n_adapters = n;
	c->adapter_bytes = total;
	c->score_cutoff = score_cutoff;
	c->adapters_set = true;
	return DBGK_OK;
}

// The batch buffers are the handle's INPUT side only: the compact batch and a pending push live in buffers of their own (emit), and a
// gather has finished when dbgk_clean_compact returns, so regrowing here never frees what either still needs.
static int clean_ensure_batch(dbgk_clean *c, uint64_t n_bytes, uint64_t n_reads, bool with_qual)
{
	if (n_bytes + 16 > c->cap_bytes || n_reads > c->cap_reads || (with_qual && c->cap_qual < c->cap_bytes)) {
		const uint64_t bytes = std::max<uint64_t>(std::max<uint64_t>(n_bytes + 16, c->cap_bytes), 1 << 20);
		const uint64_t reads = std::max<uint64_t>(std::max<uint64_t>(n_reads, c->cap_reads), 1 << 14);
		const bool qual = with_qual || c->cap_qual;
		c->cap_bytes = c->cap_qual = c->cap_reads = 0;
		if (c->d_seq.reserve(bytes) || (qual && c->d_qual.reserve(bytes)) || c->d_off.reserve((reads + 1) * 8) || c->d_out.reserve(reads * 24) ||
		    c->d_long.reserve(reads * 4))
			return DBGK_ERR_NOMEM;
		c->cap_bytes = bytes;
		c->cap_qual = qual ? bytes : 0;
		c->cap_reads = reads;
	}
	return DBGK_OK;
}

// a plane handed to a _device call: 16-byte aligned, and not one of the handle's own compact planes
static bool clean_device_plane_ok(const dbgk_clean *c, const char *p)
{
	if ((uintptr_t)p & 15u) return false;
	const uint8_t *u = (const uint8_t *)p;
	for (const uint8_t *own : {c->emit.bases.p, c->emit.quals.p})
		if (u && own && u >= own && u < own + c->emit.cap_bytes) return false;
	return true;
}

// the batch that d_off / d_out now describe: n reads of the planes seq / qual (qual null: no quality plane)
static void clean_batch_is(dbgk_clean *c, int32_t kind, int32_t shift, uint64_t n, const uint8_t *seq, const uint8_t *qual)
{
	c->have_batch = true;
	c->batch_n = n;
	c->batch_kind = kind;
	c->batch_shift = shift;
	c->b_seq = seq;
	c->b_qual = qual;
}

// dbgk_clean_adapter (on_device: dbgk_clean_adapter_device, `bases` and `d_quals` are device memory and only the upload is skipped)
static int clean_adapter_run(dbgk_clean *c, const char *bases, bool on_device, const char *d_quals, const uint64_t *offsets, uint64_t n_reads,
                             dbgk_adapter_hit *out)
{
	if (!c || (n_reads && !out)) return DBGK_ERR_ARG;
	uint64_t max_len = 0;
	int rc = cleank::clean_check_batch(offsets, n_reads, &max_len);
	if (rc) return rc;
	if (n_reads && offsets[n_reads] && !bases) return DBGK_ERR_ARG;
	if (on_device && (!clean_device_plane_ok(c, bases) || !clean_device_plane_ok(c, d_quals))) return DBGK_ERR_ARG;
	if (!c->adapters_set) return DBGK_ERR_STATE;
	c->last = dbgk_clean_stats{};
	c->last.reads = n_reads;
	c->have_batch = c->emit.have = false;
	if (!n_reads) {
		clean_batch_is(c, DBGK_CLEAN_KIND_ADAPTER, 0, 0, nullptr, nullptr);
		return DBGK_OK;
	}
	HIPCHK(hipSetDevice(c->device));
	const uint64_t nb = offsets[n_reads];
	rc = clean_ensure_batch(c, on_device ? 0 : nb, n_reads, false);
	if (rc) return rc;
	if (nb && !on_device) HIPCHK(hipMemcpyAsync(c->d_seq, bases, nb, hipMemcpyHostToDevice, c->stream));
	const uint8_t *d_in = on_device ? (const uint8_t *)bases : c->d_seq.p;
	HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(c->d_ctr, 0, sizeof(cleank::CleanCounters), c->stream));
	cleank::AdapterHit *d_hits = reinterpret_cast<cleank::AdapterHit *>(c->d_out.p);
	const uint32_t nr = (uint32_t)n_reads, n_ad = (uint32_t)c->n_adapters;
	const bool lds_form = c->adapter_bytes <= cleank::kCleanAdapterBytes;
	auto grid_for = [&](uint64_t items) {
		return (unsigned)std::min<uint64_t>((items + cleank::kCleanWaves - 1) / cleank::kCleanWaves, (uint64_t)c->n_cu * 32);
	};
	cleank::CleanCounters hc{};
	if (lds_form) {
		HIPCHK(hipEventRecord(c->ev[0], c->stream));
		hipLaunchKernelGGL(cleank::k_clean_adapter<false>, dim3(grid_for(n_reads)), dim3(cleank::kCleanWaves * 64), 0, c->stream, d_in, c->d_off,
		                   nr, c->d_ad, c->d_ad_off, n_ad, c->score_cutoff, 0u, d_hits, c->d_long, c->d_ctr);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(c->ev[1], c->stream));
		HIPCHK(hipMemcpyAsync(&hc, c->d_ctr, sizeof hc, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	const uint64_t n_global = lds_form ? hc.n_long : n_reads; // reads beyond the LDS slice, or an adapter set beyond the LDS form
	if (n_global) {
		HIPCHK(hipEventRecord(c->ev[2], c->stream));
		hipLaunchKernelGGL(cleank::k_clean_adapter<true>, dim3(grid_for(n_global)), dim3(cleank::kCleanWaves * 64), 0, c->stream, d_in, c->d_off,
		                   nr, c->d_ad, c->d_ad_off, n_ad, c->score_cutoff, lds_form ? 1u : 0u, d_hits, c->d_long, c->d_ctr);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(c->ev[3], c->stream));
		HIPCHK(hipMemcpyAsync(&hc, c->d_ctr, sizeof hc, hipMemcpyDeviceToHost, c->stream));
	}
	HIPCHK(hipMemcpyAsync(out, d_hits, n_reads * sizeof(cleank::AdapterHit), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	float ms = 0;
	if (lds_form) {
		HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
		c->last.ms_lds = ms;
	}
	if (n_global) {
		HIPCHK(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
		c->last.ms_global = ms;
	}
	c->last.by_lds = hc.by_lds;
	c->last.by_global = hc.by_global;
	c->last.hits = hc.hits;
	c->last.cells = hc.cells;
	clean_batch_is(c, DBGK_CLEAN_KIND_ADAPTER, 0, n_reads, d_in, on_device ? (const uint8_t *)d_quals : nullptr);
	return DBGK_OK;
}

extern "C" int dbgk_clean_adapter(dbgk_clean *c, const char *bases, const uint64_t *offsets, uint64_t n_reads, dbgk_adapter_hit *out)
{
	return clean_adapter_run(c, bases, false, nullptr, offsets, n_reads, out);
}

extern "C" int dbgk_clean_adapter_device(dbgk_clean *c, const char *d_bases, const char *d_quals, const uint64_t *offsets, uint64_t n_reads,
                                         dbgk_adapter_hit *out)
{
	return clean_adapter_run(c, d_bases, true, d_quals, offsets, n_reads, out);
}

// dbgk_clean_lowqual (on_device: dbgk_clean_lowqual_device, `bases` and `quals` are device memory and only the upload is skipped)
static int clean_lowqual_run(dbgk_clean *c, const char *bases, const char *quals, bool on_device, const uint64_t *offsets, uint64_t n_reads,
                             double error_rate_cutoff, int32_t quality_shift, dbgk_lowqual_block *out)
{
	if (!c || (n_reads && !out) || error_rate_cutoff != error_rate_cutoff || quality_shift < 0 || quality_shift > 127) return DBGK_ERR_ARG;
	uint64_t max_len = 0;
	int rc = cleank::clean_check_batch(offsets, n_reads, &max_len);
	if (rc) return rc;
	if (n_reads && offsets[n_reads] && (!bases || !quals)) return DBGK_ERR_ARG;
	if (on_device && (!clean_device_plane_ok(c, bases) || !clean_device_plane_ok(c, quals))) return DBGK_ERR_ARG;
	c->last = dbgk_clean_stats{};
	c->last.reads = n_reads;
	c->have_batch = c->emit.have = false;
	if (!n_reads) {
		clean_batch_is(c, DBGK_CLEAN_KIND_LOWQUAL, quality_shift, 0, nullptr, nullptr);
		return DBGK_OK;
	}
	HIPCHK(hipSetDevice(c->device));
	if (c->table_shift != quality_shift) {
		// Qual2Err[i + shift] = pow(10.0, -i / 10.0), i = 0 .. 99 (clean_lowqual.cpp:220-222), with the host's libm; the entries from 128
		// on, which the reference writes behind its array and never reads, stay 0
		double table[256] = {0.0};
		for (int i = 0; i < 100; ++i)
			if (i + quality_shift < 128) table[i + quality_shift] = pow(10.0, -i / 10.0);
		HIPCHK(hipMemcpyAsync(c->d_table, table, sizeof table, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		c->table_shift = quality_shift;
	}
	const uint64_t nb = offsets[n_reads];
	rc = on_device ? clean_ensure_batch(c, 0, n_reads, false) : clean_ensure_batch(c, nb, n_reads, true);
	if (rc) return rc;
	if (nb && !on_device) {
		HIPCHK(hipMemcpyAsync(c->d_seq, bases, nb, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(c->d_qual, quals, nb, hipMemcpyHostToDevice, c->stream));
	}
	const uint8_t *d_in = on_device ? (const uint8_t *)bases : c->d_seq.p, *d_in_q = on_device ? (const uint8_t *)quals : c->d_qual.p;
	HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
	cleank::LowqualBlock *d_blocks = reinterpret_cast<cleank::LowqualBlock *>(c->d_out.p);
	const unsigned grid = (unsigned)((n_reads + cleank::kLowqualThreads - 1) / cleank::kLowqualThreads);
	HIPCHK(hipEventRecord(c->ev[0], c->stream));
	hipLaunchKernelGGL(cleank::k_clean_lowqual, dim3(grid), dim3(cleank::kLowqualThreads), 0, c->stream, d_in, d_in_q, c->d_off,
	                   (uint32_t)n_reads, c->d_table, error_rate_cutoff, (uint32_t)quality_shift, d_blocks);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(c->ev[1], c->stream));
	HIPCHK(hipMemcpyAsync(out, d_blocks, n_reads * sizeof(cleank::LowqualBlock), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
	c->last.ms_lowqual = ms;
	clean_batch_is(c, DBGK_CLEAN_KIND_LOWQUAL, quality_shift, n_reads, d_in, d_in_q);
	return DBGK_OK;
}

extern "C" int dbgk_clean_lowqual(dbgk_clean *c, const char *bases, const char *quals, const uint64_t *offsets, uint64_t n_reads,
                                  double error_rate_cutoff, int32_t quality_shift, dbgk_lowqual_block *out)
{
	return clean_lowqual_run(c, bases, quals, false, offsets, n_reads, error_rate_cutoff, quality_shift, out);
}

extern "C" int dbgk_clean_lowqual_device(dbgk_clean *c, const char *d_bases, const char *d_quals, const uint64_t *offsets, uint64_t n_reads,
                                         double error_rate_cutoff, int32_t quality_shift, dbgk_lowqual_block *out)
{
	return clean_lowqual_run(c, d_bases, d_quals, true, offsets, n_reads, error_rate_cutoff, quality_shift, out);
}

extern "C" int dbgk_clean_batch_stats(dbgk_clean *c, dbgk_clean_stats *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	*out = c->last;
	return DBGK_OK;
}

// ---- output stage: compact batch on the device, hand-over to a graph handle (dbgk_host_emit.h, kernels in dbgk_emit.h) ------------

template <int KIND>
static void clean_launch_len(dbgk_clean *c, uint32_t min_len, unsigned grid, uint32_t *len, uint64_t *src, unsigned long long *ctr)
{
	using R = emitk::CleanRule<KIND>;
	hipLaunchKernelGGL(emitk::k_emit_out_len<R>, dim3(grid), dim3(emitk::kEmitBlock), 0, c->stream, c->d_off, R{c->d_out, min_len}, (uint32_t)c->batch_n,
	                   len, src, ctr);
}

static int clean_compact_run(dbgk_clean *c, uint32_t min_len, dbgk_clean_compact_info *out)
{
	using R = emitk::CleanRule<DBGK_CLEAN_KIND_LOWQUAL>; // (the counters of both kinds)
	const bool lowqual = c->batch_kind == DBGK_CLEAN_KIND_LOWQUAL;
	HIPCHK(hipSetDevice(c->device));
	auto launch_len = [&](unsigned grid, uint32_t *len, uint64_t *src, unsigned long long *ctr) {
		if (lowqual) clean_launch_len<DBGK_CLEAN_KIND_LOWQUAL>(c, min_len, grid, len, src, ctr);
		else clean_launch_len<DBGK_CLEAN_KIND_ADAPTER>(c, min_len, grid, len, src, ctr);
	};
	unsigned long long ctr[R::EC_COUNT];
	dbgk_clean_compact_info I{};
	int rc = emit_run(c->emit, c->stream, c->n_cu, c->batch_n, c->b_seq, c->b_qual, lowqual, (uint32_t)c->batch_shift * 0x01010101u, launch_len, ctr,
	                  &I.ms_scan, &I.ms_gather);
	if (rc) return rc;
	I.reads = c->batch_n;
	I.raw_bases = ctr[R::EC_RAW_BASES];
	I.trimmed_reads = ctr[R::EC_TRIMMED_READS];
	I.trimmed_bases = ctr[R::EC_TRIMMED_BASES];
	I.short_reads = ctr[R::EC_SHORT_READS];
	I.short_bases = ctr[R::EC_SHORT_BASES];
	I.clean_reads = ctr[R::EC_CLEAN_READS];
	I.clean_bases = ctr[R::EC_CLEAN_BASES];
	*out = I;
	return DBGK_OK;
}

extern "C" int dbgk_clean_compact(dbgk_clean *c, int32_t min_len, dbgk_clean_compact_info *out)
{
	if (!c || !out || min_len < 0) return DBGK_ERR_ARG;
	if (!c->have_batch) return DBGK_ERR_STATE;
	return clean_compact_run(c, (uint32_t)min_len, out);
}

extern "C" int dbgk_clean_compact_from(dbgk_clean *c, int32_t kind, const char *bases, const char *quals, const uint64_t *offsets,
                                       const void *recs, uint64_t n_reads, int32_t quality_shift, int32_t min_len, dbgk_clean_compact_info *out)
{
	if (!c || !out || min_len < 0 || (kind != DBGK_CLEAN_KIND_LOWQUAL && kind != DBGK_CLEAN_KIND_ADAPTER)) return DBGK_ERR_ARG;
	if (kind == DBGK_CLEAN_KIND_LOWQUAL && (quality_shift < 0 || quality_shift > 127)) return DBGK_ERR_ARG;
	uint64_t max_len = 0;
	int rc = cleank::clean_check_batch(offsets, n_reads, &max_len);
	if (rc) return rc;
	if (n_reads && (!recs || (offsets[n_reads] && !bases))) return DBGK_ERR_ARG;
	c->last = dbgk_clean_stats{};
	c->last.reads = n_reads;
	c->have_batch = c->emit.have = false;
	HIPCHK(hipSetDevice(c->device));
	const uint64_t nb = n_reads ? offsets[n_reads] : 0;
	if (n_reads) {
		rc = clean_ensure_batch(c, nb, n_reads, quals != nullptr);
		if (rc) return rc;
		if (nb) {
			HIPCHK(hipMemcpyAsync(c->d_seq, bases, nb, hipMemcpyHostToDevice, c->stream));
			if (quals) HIPCHK(hipMemcpyAsync(c->d_qual, quals, nb, hipMemcpyHostToDevice, c->stream));
		}
		HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(c->d_out, recs, n_reads * 24, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream)); // the caller's buffers are free on return
	}
	clean_batch_is(c, kind, kind == DBGK_CLEAN_KIND_LOWQUAL ? quality_shift : 0, n_reads, n_reads ? c->d_seq.p : nullptr,
	               n_reads && quals ? c->d_qual.p : nullptr);
	return clean_compact_run(c, (uint32_t)min_len, out);
}

extern "C" int dbgk_clean_compact_results(dbgk_clean *c, char *bases, char *quals, uint64_t *offsets)
{
	if (!c) return DBGK_ERR_ARG;
	if (!c->emit.have) return DBGK_ERR_STATE;
	if (quals && !c->emit.has_qual) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(c->device));
	return emit_results(c->emit, c->stream, bases, quals, offsets);
}

extern "C" int dbgk_clean_compact_device(dbgk_clean *c, const char **d_bases, const char **d_quals, const uint64_t **d_offsets,
                                         uint64_t *n_reads, uint64_t *n_bases)
{
	if (!c || !d_bases || !d_quals || !d_offsets || !n_reads || !n_bases) return DBGK_ERR_ARG;
	if (!c->emit.have) return DBGK_ERR_STATE;
	emit_device(c->emit, d_bases, d_quals, d_offsets, n_reads, n_bases);
	return DBGK_OK;
}

extern "C" int dbgk_push_cleaned(dbgk_handle *h, dbgk_clean *c)
{
	if (!h || !c) return DBGK_ERR_ARG;
	if (h->device != c->device) return DBGK_ERR_ARG;
	return emit_push(h, c->emit);
}
