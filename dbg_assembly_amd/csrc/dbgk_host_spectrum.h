// SPECTRUM: host side of the k-mer frequency spectrum and of simulate_lowfreq_kmer's scan (kernels in dbgk_spectrum.h)

// bins 1..255 of counts[first, first + n) of one handle added to acc[1..255]; the caller derives bin 0.  The device bins and the
// two events around the kernel belong to the handle and are made at the first call.
static int kfreq_spectrum_add(dbgk_handle *h, uint64_t first, uint64_t n, uint64_t acc[256])
{
	int rc = use_device(h);
	if (rc) return rc;
	h->kf_spectrum_ms = 0;
	if (n == 0) return DBGK_OK;
	if (h->kf_bins.reserve(256 * sizeof(unsigned long long))) return DBGK_ERR_NOMEM;
	for (StageEvent &e : h->kf_ev)
		if (e.create()) return DBGK_ERR_HIP;
	unsigned long long bins[256];
	HIPCHK(hipMemsetAsync(h->kf_bins, 0, sizeof bins, h->stream));
	// a workgroup's 32-bit LDS bins hold what it reads: fewer than 2^31 bytes each, however few CUs there are
	const uint64_t per_pass = (uint64_t)spec::kThreads * spec::kInFlight * 16;
	uint64_t grid = std::min<uint64_t>((n + per_pass - 1) / per_pass, (uint64_t)std::max(h->n_cu, 1) * 8);
	grid = std::max<uint64_t>(grid, (n >> 31) + 1);
	HIPCHK(hipEventRecord(h->kf_ev[0], h->stream));
	hipLaunchKernelGGL(spec::k_kf_spectrum, dim3((unsigned)grid), dim3(spec::kThreads), 0, h->stream, (const uint8_t *)h->counts, first, n,
	                   h->kf_bins);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(h->kf_ev[1], h->stream));
	HIPCHK(hipMemcpyAsync(bins, h->kf_bins, sizeof bins, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, h->kf_ev[0], h->kf_ev[1]));
	h->kf_spectrum_ms = ms;
	for (int c = 1; c < 256; ++c) acc[c] += bins[c];
	return DBGK_OK;
}

static void kfreq_spectrum_bin0(uint64_t n, uint64_t hist[256])
{
	uint64_t nonzero = 0;
	for (int c = 1; c < 256; ++c) nonzero += hist[c];
	hist[0] = n - nonzero;
}

extern "C" int dbgk_kfreq_spectrum(dbgk_handle *h, uint64_t first_kmer, uint64_t n, uint64_t hist[256])
{
	if (!h || !hist) return DBGK_ERR_ARG;
	if (!h->kfreq || !h->finalized) return DBGK_ERR_STATE;
	const uint64_t total = 1ull << (2 * h->cfg.kmer_size);
	if (first_kmer > total || n > total - first_kmer) return DBGK_ERR_ARG;
	memset(hist, 0, 256 * sizeof(uint64_t));
	const int rc = kfreq_spectrum_add(h, first_kmer, n, hist);
	if (rc) return rc;
	kfreq_spectrum_bin0(n, hist);
	return DBGK_OK;
}

extern "C" int dbgk_kfreq_spectrum_ms(dbgk_handle *h, double *ms)
{
	if (!h || !ms) return DBGK_ERR_ARG;
	if (!h->kfreq) return DBGK_ERR_STATE;
	*ms = h->kf_spectrum_ms;
	return DBGK_OK;
}

// the table of the whole job: every member over the range it owns
extern "C" int dbgk_comm_kfreq_spectrum(dbgk_comm *c, uint64_t hist[256])
{
	if (!c || !hist) return DBGK_ERR_ARG;
	if (!c->kfreq || !c->finalized) return DBGK_ERR_STATE;
	memset(hist, 0, 256 * sizeof(uint64_t));
	for (size_t d = 0; d < c->h.size(); d++) {
		const int rc = kfreq_spectrum_add(c->h[d], c->kf_lo[d], c->kf_lo[d + 1] - c->kf_lo[d], hist);
		if (rc) return rc;
	}
	kfreq_spectrum_bin0(1ull << (2 * c->h[0]->cfg.kmer_size), hist); // (the members' ranges cover the padding of k < 3 too: zeros)
	return DBGK_OK;
}

extern "C" int dbgk_corr_mutation_scan(dbgk_corr *c, const char *seq, const uint64_t *offsets, uint64_t n_seqs, uint32_t skip,
                                       uint64_t *hist)
{
	if (!c || !offsets || !hist || skip == 0 || (n_seqs && !seq)) return DBGK_ERR_ARG;
	if (!c->sealed) return DBGK_ERR_STATE;
	if (offsets[0] != 0) return DBGK_ERR_ARG;
	const int k = c->p.k;
	const uint64_t frag = 2 * (uint64_t)k - 1;
	std::vector<uint64_t> site_lo(n_seqs + 1, 0);
	for (uint64_t i = 0; i < n_seqs; ++i) {
		if (offsets[i + 1] < offsets[i]) return DBGK_ERR_ARG;
		const uint64_t len = offsets[i + 1] - offsets[i];
		site_lo[i + 1] = site_lo[i] + (len >= frag ? (len - frag) / skip + 1 : 0);
	}
	memset(hist, 0, (size_t)(k + 1) * sizeof(uint64_t));
	c->ms_mut_scan = 0;
	const uint64_t n_sites = site_lo[n_seqs];
	if (n_sites == 0) return DBGK_OK;
	int rc = corr_use(c);
	if (rc) return rc;
	const uint64_t nb = offsets[n_seqs];
	DevBuf<uint8_t> d_seq;
	DevBuf<uint64_t> d_off; // offsets, then site_lo, then the k + 1 bins
	const uint64_t words = 2 * (n_seqs + 1) + (uint64_t)k + 1;
	if (d_seq.reserve(nb) || d_off.reserve(words * 8)) return DBGK_ERR_NOMEM;
	uint64_t *d_lo = d_off + (n_seqs + 1);
	unsigned long long *d_hist = (unsigned long long *)(d_lo + (n_seqs + 1));
	HIPCHK(hipMemcpyAsync(d_seq, seq, nb, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_lo, site_lo.data(), (n_seqs + 1) * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)(k + 1) * 8, c->stream));
	float ms = 0;
	uint32_t steps = 1;
	while ((n_seqs >> steps) != 0) ++steps; // halvings that bring a range of n_seqs down to one
	const uint64_t grid = std::min<uint64_t>((n_sites + spec::kThreads - 1) / spec::kThreads, (uint64_t)std::max(c->n_cu, 1) * 16);
	(void)hipEventRecord(c->ev[0], c->stream);
	hipLaunchKernelGGL(spec::k_mut_scan, dim3((unsigned)grid), dim3(spec::kThreads), 0, c->stream, (const uint8_t *)d_seq,
	                   (const uint64_t *)d_off, (const uint64_t *)d_lo, n_seqs, steps, n_sites, skip, k, (const uint32_t *)c->tab,
	                   c->cp.total, d_hist);
	HIPCHK(hipGetLastError());
	(void)hipEventRecord(c->ev[1], c->stream);
	HIPCHK(hipMemcpyAsync(hist, d_hist, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->ms_mut_scan = ms;
	return DBGK_OK;
}

extern "C" int dbgk_corr_mutation_scan_ms(dbgk_corr *c, double *ms)
{
	if (!c || !ms) return DBGK_ERR_ARG;
	*ms = c->ms_mut_scan;
	return DBGK_OK;
}
