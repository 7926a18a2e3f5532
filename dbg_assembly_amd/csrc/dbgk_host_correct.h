// CORRECT: host side of correct_error_reads on the GPU (include/dbgk.h, ABI 7; kernels in dbgk_correct.h)

struct dbgk_corr : StageDev {
	dbgk_corr_params p{};
	corr::CorrParams cp{};
	DevBuf<uint32_t> tab;         // the loaded table, ceil(4^k / 32) words
	uint64_t tab_words = 0;
	bool sealed = false;
	uint64_t hifreq = 0;
	// batch buffers, grown on demand
	DevBuf<uint8_t> d_seq, d_out, d_scratch;
	DevBuf<uint64_t> d_off;
	DevBuf<dbgk_corr_rec> d_rec;
	DevBuf<uint32_t> d_work, d_ovf;
	DevBuf<uint64_t> d_cnt;
	uint64_t cap_bytes = 0, cap_reads = 0;
	StageEvents<4> ev;
	dbgk_corr_stats last{};
	double ms_mut_scan = 0;       // device time of the last k_mut_scan
	// output stage (dbgk_host_emit.h): the batch d_out / d_off / d_rec hold, and its compact form
	bool have_batch = false;      // the last dbgk_corr_reads* / dbgk_corr_compact_from succeeded: batch_n reads are resident
	uint64_t batch_n = 0;
	EmitStage emit;
	AnnotStage annot;             // the headers' annotation of the compact batch (dbgk_host_annot.h)
};

static int corr_use(dbgk_corr *c)
{
	HIPCHK(hipSetDevice(c->device));
	return DBGK_OK;
}

extern "C" int dbgk_corr_create(const dbgk_corr_params *p, int device, dbgk_corr **out)
{
	if (!p || !out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (p->k < 1 || p->k > 19 || p->min_high_region < 1 || p->max_change < 0 || p->further_trim < 0 ||
	    p->max_tree_nodes < 1 || p->max_tree_nodes >= (1 << 26) || p->min_trimmed_len < 0 || device < 0)
		return DBGK_ERR_ARG;
	dbgk_corr *c = new (std::nothrow) dbgk_corr;
	if (!c) return DBGK_ERR_NOMEM;
	c->p = *p;
	c->cp = corr::CorrParams{p->k, p->min_high_region, p->max_change, p->further_trim, p->max_tree_nodes, p->min_trimmed_len,
	                         1ull << (2 * p->k)};
	c->tab_words = (c->cp.total + 31) / 32;
	int rc = stage_open(*c, device);
	if (!rc) rc = c->ev.create();
	if (!rc) rc = emit_create(c->emit, emitk::CorrRule::kCounters, true);
	if (!rc) rc = c->annot.ev.create();
	if (!rc) rc = c->tab.reserve(c->tab_words * 4);
	if (!rc) rc = c->d_cnt.reserve(4 * sizeof(uint64_t));
	if (!rc && hipMemsetAsync(c->tab, 0, c->tab_words * 4, c->stream) != hipSuccess) rc = DBGK_ERR_HIP;
	if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = DBGK_ERR_HIP;
	if (rc) {
		dbgk_corr_destroy(c);
		return rc;
	}
	*out = c;
	return DBGK_OK;
}

extern "C" int dbgk_corr_destroy(dbgk_corr *c)
{
	if (!c) return DBGK_ERR_ARG;
	stage_drain(c->device, c->stream);
	emit_destroy(c->emit);
	delete c;
	return DBGK_OK;
}

extern "C" int dbgk_corr_load_bits(dbgk_corr *c, uint64_t first_byte, uint64_t n_bytes, const uint8_t *host_bits)
{
	if (!c || (!host_bits && n_bytes)) return DBGK_ERR_ARG;
	if (c->sealed) return DBGK_ERR_STATE;
	const uint64_t bytes = c->tab_words * 4;
	if (first_byte > bytes || n_bytes > bytes - first_byte) return DBGK_ERR_ARG;
	int rc = corr_use(c);
	if (rc) return rc;
	if (!n_bytes) return DBGK_OK;
	HIPCHK(hipMemcpyAsync((uint8_t *)c->tab.p + first_byte, host_bits, n_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DBGK_OK;
}

static int corr_table_kernel_done(dbgk_corr *c, unsigned long long *d_hif)
{
	HIPCHK(hipGetLastError());
	unsigned long long h = 0;
	HIPCHK(hipMemcpyAsync(&h, d_hif, sizeof h, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->hifreq = h;
	c->sealed = true;
	return DBGK_OK;
}

static unsigned corr_table_grid(const dbgk_corr *c)
{
	const uint64_t want = (c->tab_words + 255) / 256;
	return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)c->n_cu * 16));
}

extern "C" int dbgk_corr_seal(dbgk_corr *c)
{
	if (!c) return DBGK_ERR_ARG;
	if (c->sealed) return DBGK_ERR_STATE;
	int rc = corr_use(c);
	if (rc) return rc;
	unsigned long long *d_hif = (unsigned long long *)c->d_cnt.p;
	HIPCHK(hipMemsetAsync(d_hif, 0, sizeof *d_hif, c->stream));
	hipLaunchKernelGGL(corr::k_corr_seal, dim3(corr_table_grid(c)), dim3(256), 0, c->stream, c->tab, c->tab_words, c->cp.total,
	                   c->p.k, d_hif);
	return corr_table_kernel_done(c, d_hif);
}

extern "C" int dbgk_corr_from_kfreq(dbgk_corr *c, dbgk_handle *h, uint32_t cutoff)
{
	if (!c || !h) return DBGK_ERR_ARG;
	if (!h->kfreq || !h->finalized || c->sealed) return DBGK_ERR_STATE;
	// (a KFREQ table of k < 3 is padded to 64 counters: only the first 4^k are read)
	if (h->cfg.kmer_size != c->p.k || h->device != c->device || h->n_counts != std::max<uint64_t>(c->cp.total, 64)) return DBGK_ERR_ARG;
	int rc = corr_use(c);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(h->stream)); // the counts are final on the handle's stream
	unsigned long long *d_hif = (unsigned long long *)c->d_cnt.p;
	HIPCHK(hipMemsetAsync(d_hif, 0, sizeof *d_hif, c->stream));
	hipLaunchKernelGGL(corr::k_corr_from_counts, dim3(corr_table_grid(c)), dim3(256), 0, c->stream, c->tab, c->tab_words,
	                   c->cp.total, c->p.k, (const uint8_t *)h->counts, cutoff, d_hif);
	return corr_table_kernel_done(c, d_hif);
}

extern "C" int dbgk_corr_table_stats(dbgk_corr *c, uint64_t *theory_total, uint64_t *hifreq)
{
	if (!c || !theory_total || !hifreq) return DBGK_ERR_ARG;
	if (!c->sealed) return DBGK_ERR_STATE;
	*theory_total = c->cp.total;
	*hifreq = c->hifreq;
	return DBGK_OK;
}

extern "C" int dbgk_corr_export_bits(dbgk_corr *c, uint64_t first_byte, uint64_t n_bytes, uint8_t *host_out)
{
	if (!c || (!host_out && n_bytes)) return DBGK_ERR_ARG;
	if (!c->sealed) return DBGK_ERR_STATE;
	const uint64_t bytes = c->tab_words * 4;
	if (first_byte > bytes || n_bytes > bytes - first_byte) return DBGK_ERR_ARG;
	int rc = corr_use(c);
	if (rc) return rc;
	if (!n_bytes) return DBGK_OK;
	HIPCHK(hipMemcpyAsync(host_out, (const uint8_t *)c->tab.p + first_byte, n_bytes, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DBGK_OK;
}

// frontier bound of a tree over d cycles: a node is its path, and a path is fixed by its <= 2 edits (4 bases each)
static uint64_t corr_frontier_bound(uint64_t d) { return 1 + 4 * d + 8 * d * (d > 0 ? d - 1 : 0); }

// validation of a batch's offsets and the batch buffers, grown on demand: what dbgk_corr_reads does before its upload
static int corr_batch_begin(dbgk_corr *c, const uint64_t *offsets, uint64_t n)
{
	if (offsets[0] != 0 || n >= (1ull << 32)) return DBGK_ERR_ARG;
	uint64_t max_len = 0;
	for (uint64_t i = 0; i < n; ++i) {
		if (offsets[i + 1] < offsets[i]) return DBGK_ERR_ARG;
		max_len = std::max<uint64_t>(max_len, offsets[i + 1] - offsets[i]);
	}
	if (max_len >= (1ull << 29)) return DBGK_ERR_ARG;
	c->last = dbgk_corr_stats{};
	c->last.reads = n;
	c->have_batch = c->emit.have = c->annot.have = false;
	if (!n) return DBGK_OK;
	int rc = corr_use(c);
	if (rc) return rc;
	const uint64_t nb = offsets[n];
	if (nb + 16 > c->cap_bytes || n > c->cap_reads) {
		const uint64_t bytes = std::max<uint64_t>(nb + 16, 1 << 20), reads = std::max<uint64_t>(n, 1 << 14);
		c->cap_bytes = c->cap_reads = 0;
		if (c->d_seq.reserve(bytes) || c->d_out.reserve(bytes) || c->d_off.reserve((reads + 1) * 8) || c->d_rec.reserve(reads * sizeof(dbgk_corr_rec)) ||
		    c->d_work.reserve(reads * 4) || c->d_ovf.reserve(reads * 4))
			return DBGK_ERR_NOMEM;
		c->cap_bytes = bytes;
		c->cap_reads = reads;
	}
	return DBGK_OK;
}

// The body of dbgk_corr_reads between its upload and its download: the three kernels over the n >= 1 reads of d_in (device memory,
// read only), whose offsets are in c->d_off already (queued on the stream) and on the host.  Corrected bytes -> c->d_out,
// records -> c->d_rec; the stream is NOT idle on return when the overflow kernel ran.
static int corr_batch_kernels(dbgk_corr *c, const uint8_t *d_in, const uint64_t *offsets, uint64_t n, uint32_t *h_cnt)
{
	uint32_t *cnt = (uint32_t *)(c->d_cnt + 2); // [0] work list length, [1] overflow list length
	HIPCHK(hipMemsetAsync(cnt, 0, 8, c->stream));
	const uint32_t nr = (uint32_t)n;
	const unsigned grid_cls = (unsigned)std::min<uint64_t>((n + 3) / 4, (uint64_t)c->n_cu * 32);
	HIPCHK(hipEventRecord(c->ev[0], c->stream));
	hipLaunchKernelGGL(corr::k_corr_classify, dim3(grid_cls), dim3(256), 0, c->stream, d_in, c->d_off, nr, c->cp,
	                   c->tab, c->d_out, c->d_rec, c->d_work, cnt);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(c->ev[1], c->stream));
	const unsigned grid_fix = (unsigned)std::min<uint64_t>(n, (uint64_t)c->n_cu * 32);
	hipLaunchKernelGGL(corr::k_corr_fix, dim3(grid_fix), dim3(corr::kWave), 0, c->stream, d_in, c->d_off, c->cp,
	                   c->tab, c->d_out, c->d_rec, c->d_work, c->d_ovf, cnt);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(c->ev[2], c->stream));
	h_cnt[0] = h_cnt[1] = 0;
	HIPCHK(hipMemcpyAsync(h_cnt, cnt, 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
	c->last.ms_classify = ms;
	HIPCHK(hipEventElapsedTime(&ms, c->ev[1], c->ev[2]));
	c->last.ms_correct = ms;
	if (h_cnt[1]) {
		// the overflow reads: a slice of global memory per wave, frontier capacity sized from -n and the read length
		std::vector<uint32_t> ids(h_cnt[1]);
		HIPCHK(hipMemcpy(ids.data(), c->d_ovf, ids.size() * 4, hipMemcpyDeviceToHost));
		uint64_t ol = 0;
		for (uint32_t i : ids) ol = std::max<uint64_t>(ol, offsets[i + 1] - offsets[i]);
		const uint64_t cap = std::min<uint64_t>((uint64_t)c->p.max_tree_nodes, corr_frontier_bound(ol));
		const uint64_t slice = (2 * cap * sizeof(corr::TNode) + (ol / 64 + 1) * 8 + ol + 255) & ~255ull;
		const uint64_t budget = 1ull << 30;
		const uint64_t waves = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)h_cnt[1], budget / slice, (uint64_t)c->n_cu * 8}));
		if (c->d_scratch.reserve(waves * slice)) return DBGK_ERR_NOMEM;
		HIPCHK(hipEventRecord(c->ev[2], c->stream));
		hipLaunchKernelGGL(corr::k_corr_overflow, dim3((unsigned)waves), dim3(corr::kWave), 0, c->stream, d_in,
		                   c->d_off, c->cp, c->tab, c->d_out, c->d_rec, c->d_ovf, h_cnt[1], c->d_scratch, slice, (uint32_t)ol, (uint32_t)cap);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(c->ev[3], c->stream));
	}
	return DBGK_OK;
}

// after the download (the stream is idle): the overflow kernel's time, the capacity check and the batch counters
static int corr_batch_end(dbgk_corr *c, const dbgk_corr_rec *out_rec, uint64_t n, const uint32_t *h_cnt)
{
	if (h_cnt[1]) {
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
		c->last.ms_overflow = ms;
	}
	for (uint64_t i = 0; i < n; ++i) {
		const dbgk_corr_rec &r = out_rec[i];
		if (r.path > 2) {
			g_last_error = "correct_error_reads: a tree frontier outgrew its bound in the overflow kernel";
			return DBGK_ERR_CAPACITY;
		}
		c->last.by_classify += r.path == 0;
		c->last.by_correct += r.path == 1;
		c->last.by_overflow += r.path == 2;
		c->last.node_limit_hits += r.node_limit_hits;
	}
	c->have_batch = true;
	c->batch_n = n;
	return DBGK_OK;
}

extern "C" int dbgk_corr_reads(dbgk_corr *c, const char *seq, const uint64_t *offsets, uint64_t n, char *out_seq,
                               dbgk_corr_rec *out_rec)
{
	if (!c || !offsets || (n && (!out_rec || !seq || !out_seq))) return DBGK_ERR_ARG;
	if (!c->sealed) return DBGK_ERR_STATE;
	int rc = corr_batch_begin(c, offsets, n);
	if (rc) return rc;
	const uint32_t none[2] = {0, 0};
	if (!n) return corr_batch_end(c, out_rec, 0, none);
	const uint64_t nb = offsets[n];
	HIPCHK(hipMemcpyAsync(c->d_seq, seq, nb, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
	uint32_t h_cnt[2];
	rc = corr_batch_kernels(c, c->d_seq, offsets, n, h_cnt);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(out_seq, c->d_out, nb, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(out_rec, c->d_rec, n * sizeof(dbgk_corr_rec), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return corr_batch_end(c, out_rec, n, h_cnt);
}

extern "C" int dbgk_corr_reads_device(dbgk_corr *c, const char *d_seq, const uint64_t *offsets, uint64_t n, dbgk_corr_rec *out_rec)
{
	if (!c || !offsets || (n && (!out_rec || !d_seq)) || ((uintptr_t)d_seq & 15u)) return DBGK_ERR_ARG;
	if (!c->sealed) return DBGK_ERR_STATE;
	int rc = corr_batch_begin(c, offsets, n);
	if (rc) return rc;
	const uint32_t none[2] = {0, 0};
	if (!n) return corr_batch_end(c, out_rec, 0, none);
	HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
	uint32_t h_cnt[2];
	rc = corr_batch_kernels(c, (const uint8_t *)d_seq, offsets, n, h_cnt);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(out_rec, c->d_rec, n * sizeof(dbgk_corr_rec), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return corr_batch_end(c, out_rec, n, h_cnt);
}

extern "C" int dbgk_corr_batch_stats(dbgk_corr *c, dbgk_corr_stats *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	*out = c->last;
	return DBGK_OK;
}

// ---- output stage: compact batch on the device, hand-over to a graph handle (dbgk_host_emit.h, kernels in dbgk_emit.h) ------------

static int corr_compact_run(dbgk_corr *c, dbgk_corr_compact_info *out)
{
	using R = emitk::CorrRule;
	c->annot.have = false; // (it describes the compact batch this call replaces)
	int rc = corr_use(c);
	if (rc) return rc;
	auto launch_len = [&](unsigned grid, uint32_t *len, uint64_t *src, unsigned long long *ctr) {
		hipLaunchKernelGGL(emitk::k_emit_out_len<R>, dim3(grid), dim3(emitk::kEmitBlock), 0, c->stream, c->d_off, R{c->d_rec}, (uint32_t)c->batch_n,
		                   len, src, ctr);
	};
	// What either gather asks of its source plane (dbgk_emit.h), on d_out:
	//  - d_out comes from hipMalloc, so it is 16-byte aligned, and corr_batch_begin leaves 16 bytes behind offsets[n]: the aligned
	//    dwords the gather reads lie inside [off[0] & ~3, off[n]) rounded up to whole dwords, inside the buffer;
	//  - R::out_len gives 0 whenever left_trim + right_trim >= L, so for every read that holds bytes src .. src + len lies inside
	//    the read (the src of a read of length 0 is never read);
	//  - n < 2^32 and every read shorter than 2^29 bytes (corr_batch_begin).
	unsigned long long ctr[R::EC_COUNT];
	dbgk_corr_compact_info I{};
	rc = emit_run(c->emit, c->stream, c->n_cu, c->batch_n, c->d_out, nullptr, false, 0u, launch_len, ctr, &I.ms_scan, &I.ms_gather);
	if (rc) return rc;
	I.reads = c->batch_n;
	I.result_reads = ctr[R::EC_RESULT_READS];
	I.result_bases = ctr[R::EC_RESULT_BASES];
	I.trimmed_reads = ctr[R::EC_TRIMMED_READS];
	I.trimmed_bases = ctr[R::EC_TRIMMED_BASES];
	I.deleted_reads = ctr[R::EC_DELETED_READS];
	I.one_base = ctr[R::EC_ONE_BASE];
	I.tree = ctr[R::EC_TREE];
	I.node_limit_hits = ctr[R::EC_NODE_LIMIT_HITS];
	I.by_classify = ctr[R::EC_BY_CLASSIFY];
	I.by_correct = ctr[R::EC_BY_CORRECT];
	I.by_overflow = ctr[R::EC_BY_OVERFLOW];
	*out = I;
	return DBGK_OK;
}

extern "C" int dbgk_corr_compact(dbgk_corr *c, dbgk_corr_compact_info *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	if (!c->have_batch) return DBGK_ERR_STATE;
	return corr_compact_run(c, out);
}

extern "C" int dbgk_corr_compact_from(dbgk_corr *c, const char *seq, const uint64_t *offsets, const dbgk_corr_rec *rec, uint64_t n,
                                      dbgk_corr_compact_info *out)
{
	if (!c || !offsets || !out || (n && (!rec || (!seq && offsets[n] != 0)))) return DBGK_ERR_ARG;
	int rc = corr_batch_begin(c, offsets, n);
	if (rc) return rc;
	if (n) {
		if (offsets[n]) HIPCHK(hipMemcpyAsync(c->d_out, seq, offsets[n], hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(c->d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(c->d_rec, rec, n * sizeof(dbgk_corr_rec), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream)); // the caller's buffers are free on return
	}
	const uint32_t none[2] = {0, 0};
	rc = corr_batch_end(c, rec, n, none);
	if (rc) return rc;
	return corr_compact_run(c, out);
}

extern "C" int dbgk_corr_compact_results(dbgk_corr *c, char *bases, uint64_t *offsets)
{
	if (!c || !offsets) return DBGK_ERR_ARG;
	if (!c->emit.have) return DBGK_ERR_STATE;
	if (!bases && c->emit.total) return DBGK_ERR_ARG;
	int rc = corr_use(c);
	if (rc) return rc;
	return emit_results(c->emit, c->stream, bases, nullptr, offsets);
}

extern "C" int dbgk_corr_compact_device(dbgk_corr *c, const char **d_bases, const uint64_t **d_offsets, uint64_t *n_reads, uint64_t *n_bases)
{
	if (!c || !d_bases || !d_offsets || !n_reads || !n_bases) return DBGK_ERR_ARG;
	if (!c->emit.have) return DBGK_ERR_STATE;
	emit_device(c->emit, d_bases, nullptr, d_offsets, n_reads, n_bases);
	return DBGK_OK;
}

extern "C" int dbgk_corr_annot(dbgk_corr *c, dbgk_corr_annot_info *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	c->annot.have = false;
	if (!c->emit.have) return DBGK_ERR_STATE;
	int rc = corr_use(c);
	if (rc) return rc;
	// d_rec and the compact offsets are complete: every call that writes them returns with the stream idle
	return annot_run(c->annot, c->stream, c->n_cu, c->d_rec, c->emit.off, c->emit.n, out);
}

extern "C" int dbgk_corr_annot_device(dbgk_corr *c, const char **d_suffix, const uint64_t **d_suffix_offsets, uint64_t *n, uint64_t *n_bytes)
{
	if (!c || !d_suffix || !d_suffix_offsets || !n || !n_bytes) return DBGK_ERR_ARG;
	if (!c->emit.have || !c->annot.have) return DBGK_ERR_STATE;
	*d_suffix = (const char *)c->annot.suf.p;
	*d_suffix_offsets = c->annot.off;
	*n = c->annot.n;
	*n_bytes = c->annot.total;
	return DBGK_OK;
}

extern "C" int dbgk_corr_annot_results(dbgk_corr *c, char *suffix, uint64_t *suffix_offsets)
{
	if (!c) return DBGK_ERR_ARG;
	if (!c->emit.have || !c->annot.have) return DBGK_ERR_STATE;
	int rc = corr_use(c);
	if (rc) return rc;
	if (suffix && c->annot.total) HIPCHK(hipMemcpyAsync(suffix, c->annot.suf, c->annot.total, hipMemcpyDeviceToHost, c->stream));
	if (suffix_offsets) HIPCHK(hipMemcpyAsync(suffix_offsets, c->annot.off, (c->annot.n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DBGK_OK;
}

extern "C" int dbgk_push_corrected(dbgk_handle *h, dbgk_corr *c)
{
	if (!h || !c) return DBGK_ERR_ARG;
	if (h->device != c->device) return DBGK_ERR_ARG;
	return emit_push(h, c->emit);
}
