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
	if (!rc && (hipMalloc(&c->d_ctr, sizeof(cleank::CleanCounters)) != hipSuccess || hipMalloc(&c->d_table, 256 * sizeof(double)) != hipSuccess))
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
	clean_free_batch(c);
	(void)hipFree(c->d_ad); (void)hipFree(c->d_ad_off); (void)hipFree(c->d_table); (void)hipFree(c->d_ctr);
	for (auto &e : c->ev)
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

// the checks both calls make on a batch; *max_len is the longest read
static int clean_check_batch(const uint64_t *offsets, uint64_t n_reads, uint64_t *max_len)
{
	if (!offsets || offsets[0] != 0 || n_reads >= (1ull << 31)) return DBGK_ERR_ARG;
	*max_len = 0;
	for (uint64_t i = 0; i < n_reads; ++i) {
		if (offsets[i + 1] < offsets[i]) return DBGK_ERR_ARG;
		*max_len = std::max<uint64_t>(*max_len, offsets[i + 1] - offsets[i]);
	}
	return *max_len >= (1ull << 30) ? DBGK_ERR_ARG : DBGK_OK;
}

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

extern "C" int dbgk_clean_adapter(dbgk_clean *c, const char *bases, const uint64_t *offsets, uint64_t n_reads, dbgk_adapter_hit *out)
{
	if (!c || (n_reads && !out)) return DBGK_ERR_ARG;
	uint64_t max_len = 0;
	int rc = clean_check_batch(offsets, n_reads, &max_len);
	if (rc) return rc;
	if (n_reads && offsets[n_reads] && !bases) return DBGK_ERR_ARG;
	if (!c->adapters_set) return DBGK_ERR_STATE;
	c->last = dbgk_clean_stats{};
	c->last.reads = n_reads;
	if (!n_reads) return DBGK_OK;
	HIPCHK(hipSetDevice(c->device));
	const uint64_t nb = offsets[n_reads];
	rc = clean_ensure_batch(c, nb, n_reads, false);
	if (rc) return rc;
	if (nb) HIPCHK(hipMemcpyAsync(c->d_seq, bases, nb, hipMemcpyHostToDevice, c->stream));
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
		hipLaunchKernelGGL(cleank::k_clean_adapter<false>, dim3(grid_for(n_reads)), dim3(cleank::kCleanWaves * 64), 0, c->stream, c->d_seq, c->d_off,
		                   nr, c->d_ad, c->d_ad_off, n_ad, c->score_cutoff, 0u, d_hits, c->d_long, c->d_ctr);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(c->ev[1], c->stream));
		HIPCHK(hipMemcpyAsync(&hc, c->d_ctr, sizeof hc, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	const uint64_t n_global = lds_form ? hc.n_long : n_reads; // reads beyond the LDS slice, or an adapter set beyond the LDS form
	if (n_global) {
		HIPCHK(hipEventRecord(c->ev[2], c->stream));
		hipLaunchKernelGGL(cleank::k_clean_adapter<true>, dim3(grid_for(n_global)), dim3(cleank::kCleanWaves * 64), 0, c->stream, c->d_seq, c->d_off,
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
	return DBGK_OK;
}

extern "C" int dbgk_clean_lowqual(dbgk_clean *c, const char *bases, const char *quals, const uint64_t *offsets, uint64_t n_reads,
                                  double error_rate_cutoff, int32_t quality_shift, dbgk_lowqual_block *out)
{
	if (!c || (n_reads && !out) || error_rate_cutoff != error_rate_cutoff || quality_shift < 0 || quality_shift > 127) return DBGK_ERR_ARG;
	uint64_t max_len = 0;
	int rc = clean_check_batch(offsets, n_reads, &max_len);
	if (rc) return rc;
	if (n_reads && offsets[n_reads] && (!bases || !quals)) return DBGK_ERR_ARG;
	c->last = dbgk_clean_stats{};
	c->last.reads = n_reads;
	if (!n_reads) return DBGK_OK;
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
	rc = clean_ensure_batch(c, nb, n_reads, true);
	if (rc) return rc;
	if (nb) {
		HIPCHK(hipMemcpyAsync(c->d_seq, bases, nb, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(c->d_qual, quals, nb, hipMemcpyHostToDevice, c->stream));
	}
	HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
	cleank::LowqualBlock *d_blocks = static_cast<cleank::LowqualBlock *>(c->d_out);
	const unsigned grid = (unsigned)((n_reads + cleank::kLowqualThreads - 1) / cleank::kLowqualThreads);
	HIPCHK(hipEventRecord(c->ev[0], c->stream));
	hipLaunchKernelGGL(cleank::k_clean_lowqual, dim3(grid), dim3(cleank::kLowqualThreads), 0, c->stream, c->d_seq, c->d_qual, c->d_off,
	                   (uint32_t)n_reads, c->d_table, error_rate_cutoff, (uint32_t)quality_shift, d_blocks);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(c->ev[1], c->stream));
	HIPCHK(hipMemcpyAsync(out, d_blocks, n_reads * sizeof(cleank::LowqualBlock), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
	c->last.ms_lowqual = ms;
	return DBGK_OK;
}

extern "C" int dbgk_clean_batch_stats(dbgk_clean *c, dbgk_clean_stats *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	*out = c->last;
	return DBGK_OK;
}
