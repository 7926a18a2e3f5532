// CLEAN: host side of clean_adapter / clean_lowqual on the GPU (include/dbgk.h, CLEAN section; kernels in dbgk_clean.h)

struct dbgk_clean {
	int device = 0;
	int n_cu = 256;
	hipStream_t stream = nullptr;
	// the adapter set: codes back to back (padded to whole dwords), offsets[n + 1]
	uint8_t *d_ad = nullptr;
	uint32_t *d_ad_off = nullptr;
	uint64_t n_adapters = 0, adapter_bytes = 0;
	int32_t score_cutoff = 0;
	bool adapters_set = false;
	// Qual2Err of clean_lowqual.cpp:220-222 for the shift it was last built for
	double *d_table = nullptr;
	int32_t table_shift = -1;
	// batch buffers, grown on demand
	uint8_t *d_seq = nullptr, *d_qual = nullptr;
	uint64_t *d_off = nullptr;
	void *d_out = nullptr; // cleank::AdapterHit or cleank::LowqualBlock per read (both 24 bytes)
	uint32_t *d_long = nullptr;
	cleank::CleanCounters *d_ctr = nullptr;
	uint64_t cap_bytes = 0, cap_qual = 0, cap_reads = 0;
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	dbgk_clean_stats last{};
	// output stage (dbgk_clean_emit.h): the batch whose offsets and records d_off / d_out hold, and its compact form
	bool have_batch = false;      // the last batch call succeeded: batch_n reads of b_seq / b_qual are resident
	uint64_t batch_n = 0;
	int32_t batch_kind = 0;       // DBGK_CLEAN_KIND_*: what d_out holds
	int32_t batch_shift = 0;      // the quality shift of a lowqual batch
	const uint8_t *b_seq = nullptr, *b_qual = nullptr; // d_seq / d_qual, or the caller's planes of a _device call; b_qual null: no quality plane
	bool have_compact = false, c_has_qual = false;
	uint8_t *c_bases = nullptr, *c_quals = nullptr; // 16-byte vectors, the pad of the last one 0; one capacity
	uint64_t *c_off = nullptr;    // batch_n + 1 compact offsets
	uint64_t *c_src = nullptr;    // where each read's result starts in b_seq / b_qual
	uint32_t *c_len = nullptr;
	void *c_tmp = nullptr;        // the scan's temporary storage
	unsigned long long *c_ctr = nullptr; // cleank::EC_COUNT counters
	uint64_t c_cap_bytes = 0, c_cap_reads = 0, c_tmp_bytes = 0;
	uint64_t c_n = 0, c_total = 0;
	hipEvent_t c_ev[4] = {nullptr, nullptr, nullptr, nullptr}; // length + scan: [0] .. [1]; gather: [2] .. [3]
	hipEvent_t c_done = nullptr;  // the compact batch is complete (recorded on `stream`)
	hipEvent_t c_read = nullptr;  // a graph handle has read it (recorded on that handle's stream by dbgk_push_cleaned)
	bool c_lent = false;          // c_read is pending: waited for before the compact buffers are written, regrown or freed
	dbgk_clean_compact_info c_info{};
};

static_assert(sizeof(dbgk_adapter_hit) == 24 && sizeof(cleank::AdapterHit) == 24, "dbgk_adapter_hit is six int32");
static_assert(sizeof(dbgk_lowqual_block) == 24 && sizeof(cleank::LowqualBlock) == 24, "dbgk_lowqual_block layout");
static_assert(offsetof(dbgk_lowqual_block, start) == 8 && offsetof(dbgk_lowqual_block, trimmed) == 16, "dbgk_lowqual_block layout");

static void clean_free_batch(dbgk_clean *c)
{
	(void)hipFree(c->d_seq); (void)hipFree(c->d_qual); (void)hipFree(c->d_off); (void)hipFree(c->d_out); (void)hipFree(c->d_long);
	c->d_seq = c->d_qual = nullptr; c->d_off = nullptr; c->d_out = nullptr; c->d_long = nullptr;
	c->cap_bytes = c->cap_qual = c->cap_reads = 0;
}

extern "C" int dbgk_clean_create(int device, dbgk_clean **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (device < 0) return DBGK_ERR_ARG;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) {
		g_last_error = "no usable HIP device";
		return DBGK_ERR_HIP;
	}
	dbgk_clean *c = new (std::nothrow) dbgk_clean;
	if (!c) return DBGK_ERR_NOMEM;
	c->device = device;
	int rc = DBGK_OK;
	hipDeviceProp_t prop;
	if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) rc = DBGK_ERR_HIP;
	if (!rc && strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		g_last_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
		rc = DBGK_ERR_HIP;
	}
	if (!rc) c->n_cu = prop.multiProcessorCount;
	if (!rc && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) rc = DBGK_ERR_HIP;
	for (int i = 0; !rc && i < 4; ++i)
		if (hipEventCreate(&c->ev[i]) != hipSuccess) rc = DBGK_ERR_HIP;
	for (int i = 0; !rc && i < 4; ++i)
		if (hipEventCreate(&c->c_ev[i]) != hipSuccess) rc = DBGK_ERR_HIP;
	if (!rc && (hipEventCreateWithFlags(&c->c_done, hipEventDisableTiming) != hipSuccess ||
	            hipEventCreateWithFlags(&c->c_read, hipEventDisableTiming) != hipSuccess))
		rc = DBGK_ERR_HIP;
	if (!rc && (hipMalloc(&c->d_ctr, sizeof(cleank::CleanCounters)) != hipSuccess || hipMalloc(&c->d_table, 256 * sizeof(double)) != hipSuccess ||
	            hipMalloc(&c->c_ctr, cleank::EC_COUNT * sizeof(unsigned long long)) != hipSuccess))
		rc = DBGK_ERR_NOMEM;
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
	(void)hipSetDevice(c->device);
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	if (c->c_lent) (void)hipEventSynchronize(c->c_read); // a graph handle may still be reading the compact batch
	clean_free_batch(c);
	(void)hipFree(c->d_ad); (void)hipFree(c->d_ad_off); (void)hipFree(c->d_table); (void)hipFree(c->d_ctr);
	(void)hipFree(c->c_bases); (void)hipFree(c->c_quals); (void)hipFree(c->c_off); (void)hipFree(c->c_src); (void)hipFree(c->c_len);
	(void)hipFree(c->c_tmp); (void)hipFree(c->c_ctr);
	for (hipEvent_t e : {c->ev[0], c->ev[1], c->ev[2], c->ev[3], c->c_ev[0], c->c_ev[1], c->c_ev[2], c->c_ev[3], c->c_done, c->c_read})
		if (e) (void)hipEventDestroy(e);
	if (c->stream) (void)hipStreamDestroy(c->stream);
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
	(void)hipFree(c->d_ad); (void)hipFree(c->d_ad_off);
	c->d_ad = nullptr; c->d_ad_off = nullptr;
	c->adapters_set = false;
	if (hipMalloc(&c->d_ad, codes.size()) != hipSuccess || hipMalloc(&c->d_ad_off, off32.size() * 4) != hipSuccess) return DBGK_ERR_NOMEM;
	HIPCHK(hipMemcpyAsync(c->d_ad, codes.data(), codes.size(), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->d_ad_off, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->n_adapters = n;
	c->adapter_bytes = total;
	c->score_cutoff = score_cutoff;
	c->adapters_set = true;
	return DBGK_OK;
}

// The batch buffers are the handle's INPUT side only: the compact batch and a pending push live in buffers of their own (c_*), and a
// gather has finished when dbgk_clean_compact returns, so regrowing here never frees what either still needs.
static int clean_ensure_batch(dbgk_clean *c, uint64_t n_bytes, uint64_t n_reads, bool with_qual)
{
	if (n_bytes + 16 > c->cap_bytes || n_reads > c->cap_reads || (with_qual && c->cap_qual < c->cap_bytes)) {
		const uint64_t bytes = std::max<uint64_t>(std::max<uint64_t>(n_bytes + 16, c->cap_bytes), 1 << 20);
		const uint64_t reads = std::max<uint64_t>(std::max<uint64_t>(n_reads, c->cap_reads), 1 << 14);
		const bool qual = with_qual || c->cap_qual;
		clean_free_batch(c);
		if (hipMalloc(&c->d_seq, bytes) != hipSuccess || (qual && hipMalloc(&c->d_qual, bytes) != hipSuccess) ||
		    hipMalloc(&c->d_off, (reads + 1) * 8) != hipSuccess || hipMalloc(&c->d_out, reads * 24) != hipSuccess ||
		    hipMalloc(&c->d_long, reads * 4) != hipSuccess) {
			clean_free_batch(c);
			return DBGK_ERR_NOMEM;
		}
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
	for (const uint8_t *own : {c->c_bases, c->c_quals})
		if (u && own && u >= own && u < own + c->c_cap_bytes) return false;
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
	c->have_batch = c->have_compact = false;
	if (!n_reads) {
		clean_batch_is(c, DBGK_CLEAN_KIND_ADAPTER, 0, 0, nullptr, nullptr);
		return DBGK_OK;
	}
	HIPCHK(hipSetDevice(c->device));
	const uint64_t nb = offsets[n_reads];
	rc = clean_ensure_batch(c, on_device ? 0 : nb, n_reads, false);
	if (rc) return rc;
	if (nb && !on_device) HIPCHK(hipMemcpyAsync(c->d_seq, bases, nb, hipMemcpyHostToDevice, c->stream));
	const uint8_t *d_in = on_device ? (const uint8_t *)bases : c->d_seq;
	HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(c->d_ctr, 0, sizeof(cleank::CleanCounters), c->stream));
	cleank::AdapterHit *d_hits = static_cast<cleank::AdapterHit *>(c->d_out);
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
	c->have_batch = c->have_compact = false;
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
	const uint8_t *d_in = on_device ? (const uint8_t *)bases : c->d_seq, *d_in_q = on_device ? (const uint8_t *)quals : c->d_qual;
	HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
	cleank::LowqualBlock *d_blocks = static_cast<cleank::LowqualBlock *>(c->d_out);
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

// ---- output stage: compact batch on the device, hand-over to a graph handle (kernels in dbgk_clean_emit.h) -----------------------

// the compact buffers are about to be written (free_them: regrown or freed): a graph handle that was given them has to be done
static int clean_compact_reclaim(dbgk_clean *c, bool free_them)
{
	if (!c->c_lent) return DBGK_OK;
	if (free_them) {
		HIPCHK(hipEventSynchronize(c->c_read));
		c->c_lent = false;
	} else {
		HIPCHK(hipStreamWaitEvent(c->stream, c->c_read, 0)); // (stays lent: a later regrow or free still has to wait on the host)
	}
	return DBGK_OK;
}

template <bool QUAL, bool SUBST>
static void clean_launch_gather(dbgk_clean *c, unsigned grid, uint64_t total)
{
	hipLaunchKernelGGL((cleank::k_clean_gather<QUAL, SUBST>), dim3(grid), dim3(cleank::kEmitBlock), 0, c->stream, c->b_seq, c->b_qual, c->c_src,
	                   c->c_off, (uint32_t)c->batch_n, total, (uint32_t)c->batch_shift * 0x01010101u, reinterpret_cast<uint4 *>(c->c_bases),
	                   reinterpret_cast<uint4 *>(c->c_quals));
}

static int clean_compact_run(dbgk_clean *c, uint32_t min_len, dbgk_clean_compact_info *out)
{
	const uint64_t n = c->batch_n;
	const bool with_qual = c->b_qual != nullptr;
	HIPCHK(hipSetDevice(c->device));
	c->have_compact = false;
	const bool grow_reads = n > c->c_cap_reads || !c->c_off;
	int rc = clean_compact_reclaim(c, grow_reads);
	if (rc) return rc;
	if (grow_reads) {
		(void)hipFree(c->c_off); (void)hipFree(c->c_len); (void)hipFree(c->c_src);
		c->c_off = nullptr; c->c_len = nullptr; c->c_src = nullptr;
		c->c_cap_reads = 0;
		const uint64_t cap = std::max<uint64_t>(n, 1 << 14);
		if (hipMalloc(&c->c_off, (cap + 1) * 8) != hipSuccess || hipMalloc(&c->c_len, (cap + 1) * 4) != hipSuccess ||
		    hipMalloc(&c->c_src, cap * 8) != hipSuccess)
			return DBGK_ERR_NOMEM;
		c->c_cap_reads = cap;
	}
	size_t need = 0;
	if (n && dbgk_internal_scan_lengths(nullptr, &need, c->c_len, c->c_off, n + 1, c->stream)) return DBGK_ERR_HIP;
	if (need > c->c_tmp_bytes) {
		HIPCHK(hipStreamSynchronize(c->stream));
		(void)hipFree(c->c_tmp);
		c->c_tmp = nullptr;
		c->c_tmp_bytes = 0;
		if (hipMalloc(&c->c_tmp, need) != hipSuccess) return DBGK_ERR_NOMEM;
		c->c_tmp_bytes = need;
	}
	HIPCHK(hipMemsetAsync(c->c_ctr, 0, cleank::EC_COUNT * sizeof(unsigned long long), c->stream));
	HIPCHK(hipEventRecord(c->c_ev[0], c->stream));
	if (n) {
		const unsigned grid = (unsigned)std::min<uint64_t>((n + cleank::kEmitBlock) / cleank::kEmitBlock, (uint64_t)c->n_cu * 16);
		if (c->batch_kind == DBGK_CLEAN_KIND_LOWQUAL)
			hipLaunchKernelGGL(cleank::k_clean_out_len<DBGK_CLEAN_KIND_LOWQUAL>, dim3(grid), dim3(cleank::kEmitBlock), 0, c->stream, c->d_off,
			                   (const void *)c->d_out, (uint32_t)n, min_len, c->c_len, c->c_src, c->c_ctr);
		else
			hipLaunchKernelGGL(cleank::k_clean_out_len<DBGK_CLEAN_KIND_ADAPTER>, dim3(grid), dim3(cleank::kEmitBlock), 0, c->stream, c->d_off,
			                   (const void *)c->d_out, (uint32_t)n, min_len, c->c_len, c->c_src, c->c_ctr);
		HIPCHK(hipGetLastError());
		size_t bytes = c->c_tmp_bytes;
		if (dbgk_internal_scan_lengths(c->c_tmp, &bytes, c->c_len, c->c_off, n + 1, c->stream)) return DBGK_ERR_HIP;
	} else {
		HIPCHK(hipMemsetAsync(c->c_off, 0, 8, c->stream));
	}
	HIPCHK(hipEventRecord(c->c_ev[1], c->stream));
	unsigned long long ctr[cleank::EC_COUNT];
	uint64_t total = 0;
	HIPCHK(hipMemcpyAsync(&total, c->c_off + n, 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(ctr, c->c_ctr, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // the total sizes the compact planes
	// whole vectors, and room behind the end for the dword and 16-byte reads of the kernels that take a plane as their input
	const uint64_t want = ((total + 15) & ~15ull) + 64;
	if (want > c->c_cap_bytes || (with_qual && !c->c_quals)) {
		rc = clean_compact_reclaim(c, true);
		if (rc) return rc;
		const bool qual = with_qual || c->c_quals; // a handle that has held a quality plane keeps one, as the batch buffers do
		(void)hipFree(c->c_bases); (void)hipFree(c->c_quals);
		c->c_bases = c->c_quals = nullptr;
		const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(want, c->c_cap_bytes), 1 << 20);
		c->c_cap_bytes = 0;
		if (hipMalloc(&c->c_bases, cap) != hipSuccess || (qual && hipMalloc(&c->c_quals, cap) != hipSuccess)) return DBGK_ERR_NOMEM;
		c->c_cap_bytes = cap;
	}
	if (total) {
		const uint64_t tiles = (total + DBGK_CLEAN_COMPACT_TILE - 1) / DBGK_CLEAN_COMPACT_TILE;
		const unsigned grid = (unsigned)std::min<uint64_t>(tiles, (uint64_t)c->n_cu * 64);
		HIPCHK(hipEventRecord(c->c_ev[2], c->stream)); // directly in front of the kernel: the copies, the host round trip and an allocation lie before it
		if (!with_qual) clean_launch_gather<false, false>(c, grid, total);
		else if (c->batch_kind == DBGK_CLEAN_KIND_LOWQUAL) clean_launch_gather<true, true>(c, grid, total);
		else clean_launch_gather<true, false>(c, grid, total);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(c->c_ev[3], c->stream));
	}
	HIPCHK(hipEventRecord(c->c_done, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	float ms_scan = 0, ms_gather = 0;
	HIPCHK(hipEventElapsedTime(&ms_scan, c->c_ev[0], c->c_ev[1]));
	if (total) HIPCHK(hipEventElapsedTime(&ms_gather, c->c_ev[2], c->c_ev[3]));
	dbgk_clean_compact_info &I = c->c_info;
	I = dbgk_clean_compact_info{};
	I.reads = n;
	I.raw_bases = ctr[cleank::EC_RAW_BASES];
	I.trimmed_reads = ctr[cleank::EC_TRIMMED_READS];
	I.trimmed_bases = ctr[cleank::EC_TRIMMED_BASES];
	I.short_reads = ctr[cleank::EC_SHORT_READS];
	I.short_bases = ctr[cleank::EC_SHORT_BASES];
	I.clean_reads = ctr[cleank::EC_CLEAN_READS];
	I.clean_bases = ctr[cleank::EC_CLEAN_BASES];
	I.ms_scan = ms_scan;
	I.ms_gather = ms_gather; // (0 when nothing is kept: no launch)
	c->c_n = n;
	c->c_total = total;
	c->c_has_qual = with_qual;
	c->have_compact = true;
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
	c->have_batch = c->have_compact = false;
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
	clean_batch_is(c, kind, kind == DBGK_CLEAN_KIND_LOWQUAL ? quality_shift : 0, n_reads, n_reads ? c->d_seq : nullptr,
	               n_reads && quals ? c->d_qual : nullptr);
	return clean_compact_run(c, (uint32_t)min_len, out);
}

extern "C" int dbgk_clean_compact_results(dbgk_clean *c, char *bases, char *quals, uint64_t *offsets)
{
	if (!c) return DBGK_ERR_ARG;
	if (!c->have_compact) return DBGK_ERR_STATE;
	if (quals && !c->c_has_qual) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(c->device));
	if (bases && c->c_total) HIPCHK(hipMemcpyAsync(bases, c->c_bases, c->c_total, hipMemcpyDeviceToHost, c->stream));
	if (quals && c->c_total) HIPCHK(hipMemcpyAsync(quals, c->c_quals, c->c_total, hipMemcpyDeviceToHost, c->stream));
	if (offsets) HIPCHK(hipMemcpyAsync(offsets, c->c_off, (c->c_n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DBGK_OK;
}

extern "C" int dbgk_clean_compact_device(dbgk_clean *c, const char **d_bases, const char **d_quals, const uint64_t **d_offsets,
                                         uint64_t *n_reads, uint64_t *n_bases)
{
	if (!c || !d_bases || !d_quals || !d_offsets || !n_reads || !n_bases) return DBGK_ERR_ARG;
	if (!c->have_compact) return DBGK_ERR_STATE;
	*d_bases = (const char *)c->c_bases;
	*d_quals = c->c_has_qual ? (const char *)c->c_quals : nullptr;
	*d_offsets = c->c_off;
	*n_reads = c->c_n;
	*n_bases = c->c_total;
	return DBGK_OK;
}

// as dbgk_push_corrected: the push queues every kernel that reads the pushed pointers on h's stream, so the event recorded behind it
// covers every reader and no dbgk_sync is needed for any engine
extern "C" int dbgk_push_cleaned(dbgk_handle *h, dbgk_clean *c)
{
	if (!h || !c) return DBGK_ERR_ARG;
	if (h->device != c->device) return DBGK_ERR_ARG;
	if (!c->have_compact || h->finalized) return DBGK_ERR_STATE;
	int rc = use_device(h);
	if (rc) return rc;
	HIPCHK(hipStreamWaitEvent(h->stream, c->c_done, 0));
	// c_read is ONE event: a push into another handle re-records it.  That handle's stream first waits for the earlier record, so
	// the new one lies behind every reader so far, whichever handles they were pushed to.
	if (c->c_lent) HIPCHK(hipStreamWaitEvent(h->stream, c->c_read, 0));
	rc = dbgk_push_reads_device(h, (const char *)c->c_bases, c->c_off, c->c_n, c->c_total);
	// (also after a failed push: part of its work may have been queued)
	if (hipEventRecord(c->c_read, h->stream) == hipSuccess) c->c_lent = true;
	else if (rc == DBGK_OK) rc = DBGK_ERR_HIP;
	return rc;
}
