// Output stage of CORRECT and CLEAN, host side (kernels in dbgk_emit.h): the compact batch of a handle on the device, its
// read-back, and its hand-over to a graph handle.  dbgk_corr and dbgk_clean each hold one EmitStage; what describes their INPUT
// batch (have_batch, batch_n, the cleaner's kind, shift and planes) stays with them.  The parser (dbgk_host_parse.h) holds one too:
// its source is the text, where the quality line of a read lies elsewhere than its sequence line (split_src).

struct EmitStage {
	DevBuf<uint8_t> bases, quals; // 16-byte vectors, the pad of the last one 0; one capacity.  quals: from the first batch with qualities on
	DevBuf<uint64_t> off;         // n + 1 compact offsets
	DevBuf<uint64_t> src;         // where each read's result starts in the source planes
	DevBuf<uint64_t> qsrc;        // split_src: ... in the quality plane's source, where that is another place (the parser's text)
	DevBuf<uint32_t> len;
	ScanTmp tmp;                  // the scan's temporary storage
	DevBuf<unsigned long long> ctr; // n_counters counters of the producer's rule
	int n_counters = 0;
	bool lds_one_plane = false;   // a batch without qualities takes k_emit_gather_lds: the corrector's stage (dbgk_emit.h says why)
	bool split_src = false;       // each plane is gathered on its own, the quality plane from qsrc: the parser's stage (set after emit_create)
	uint64_t cap_bytes = 0, cap_reads = 0;
	uint64_t n = 0, total = 0;
	bool has_qual = false;        // the compact batch has a quality plane
	bool have = false;            // the last emit_run succeeded: n reads, total bytes per plane
	StageEvents<4> ev;            // length + scan: [0] .. [1]; gather: [2] .. [3]
	hipEvent_t done = nullptr;    // the compact batch is complete (recorded on the producer's stream)
	hipEvent_t read = nullptr;    // a graph handle has read it (recorded on that handle's stream by emit_push)
	bool lent = false;            // `read` is pending: waited for before the compact buffers are written, regrown or freed
	~EmitStage()
	{
		for (hipEvent_t e : {done, read})
			if (e) (void)hipEventDestroy(e);
	}
};

static int emit_create(EmitStage &s, int n_counters, bool lds_one_plane)
{
	s.n_counters = n_counters;
	s.lds_one_plane = lds_one_plane;
	int rc = s.ev.create();
	if (rc) return rc;
	HIPCHK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
	HIPCHK(hipEventCreateWithFlags(&s.read, hipEventDisableTiming));
	return s.ctr.reserve(n_counters * sizeof(unsigned long long));
}

// before the handle is deleted (the producer's stream is idle): a graph handle may still be reading the compact batch
static void emit_destroy(EmitStage &s)
{
	if (s.lent) (void)hipEventSynchronize(s.read);
}

// the compact buffers are about to be written (free_them: regrown or freed): a graph handle that was given them has to be done
static int emit_reclaim(EmitStage &s, hipStream_t stream, bool free_them)
{
	if (!s.lent) return DBGK_OK;
	if (free_them) {
		HIPCHK(hipEventSynchronize(s.read));
		s.lent = false;
	} else {
		HIPCHK(hipStreamWaitEvent(stream, s.read, 0)); // (stays lent: a later regrow or free still has to wait on the host)
	}
	return DBGK_OK;
}

template <bool QUAL, bool SUBST>
static void emit_launch_gather(EmitStage &s, hipStream_t stream, unsigned grid, const uint8_t *seq, const uint8_t *qual, uint32_t shift_word)
{
	hipLaunchKernelGGL((emitk::k_emit_gather<QUAL, SUBST>), dim3(grid), dim3(emitk::kEmitBlock), 0, stream, seq, qual, s.src, s.off, (uint32_t)s.n,
	                   s.total, shift_word, reinterpret_cast<uint4 *>(s.bases.p), reinterpret_cast<uint4 *>(s.quals.p));
}

// The n reads of the planes seq / qual (qual null: no quality plane; subst: the quality of a base 'N' becomes the byte of shift_word)
// -> the compact batch.  launch_len(grid, len, src, ctr) launches the producer's k_emit_out_len on `stream`.  ctr: the stage's
// n_counters counters.  What the gather needs of seq / qual: dbgk_emit.h, "Memory the gather reads".  A split_src stage: qual is
// null or seq, and launch_len also fills s.qsrc (allocated here, beside s.src) when qual is set.
template <class LaunchLen>
static int emit_run(EmitStage &s, hipStream_t stream, int n_cu, uint64_t n, const uint8_t *seq, const uint8_t *qual, bool subst, uint32_t shift_word,
                    LaunchLen launch_len, unsigned long long *ctr, double *ms_scan, double *ms_gather)
{
	const bool with_qual = qual != nullptr;
	s.have = false;
	const bool grow_reads = n > s.cap_reads || !s.off;
	int rc = emit_reclaim(s, stream, grow_reads);
	if (rc) return rc;
	if (grow_reads) {
		s.cap_reads = 0;
		const uint64_t cap = std::max<uint64_t>(n, 1 << 14);
		if (s.off.reserve((cap + 1) * 8) || s.len.reserve((cap + 1) * 4) || s.src.reserve(cap * 8) || (s.split_src && s.qsrc.reserve(cap * 8)))
			return DBGK_ERR_NOMEM;
		s.cap_reads = cap;
	}
	if (n && (rc = stage_scan_reserve(s.tmp, stream, s.len, s.off, n + 1))) return rc;
	HIPCHK(hipMemsetAsync(s.ctr, 0, s.n_counters * sizeof(unsigned long long), stream));
	HIPCHK(hipEventRecord(s.ev[0], stream));
	if (n) {
		launch_len((unsigned)std::min<uint64_t>((n + emitk::kEmitBlock) / emitk::kEmitBlock, (uint64_t)n_cu * 16), s.len, s.src, s.ctr);
		HIPCHK(hipGetLastError());
		if ((rc = stage_scan(s.tmp, stream, s.len, s.off, n + 1))) return rc;
	} else {
		HIPCHK(hipMemsetAsync(s.off, 0, 8, stream));
	}
	HIPCHK(hipEventRecord(s.ev[1], stream));
	uint64_t total = 0;
	HIPCHK(hipMemcpyAsync(&total, s.off + n, 8, hipMemcpyDeviceToHost, stream));
	HIPCHK(hipMemcpyAsync(ctr, s.ctr, s.n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
	HIPCHK(hipStreamSynchronize(stream)); // the total sizes the compact planes
	// whole vectors, and room behind the end for the dword and 16-byte reads of the kernels that take a plane as their input
	const uint64_t want = ((total + 15) & ~15ull) + 64;
	if (want > s.cap_bytes || (with_qual && !s.quals)) {
		rc = emit_reclaim(s, stream, true);
		if (rc) return rc;
		const bool keep_qual = with_qual || s.quals; // a stage that has held a quality plane keeps one, as the cleaner's batch buffers do
		const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(want, s.cap_bytes), 1 << 20);
		s.cap_bytes = 0;
		if (s.bases.reserve(cap) || (keep_qual && s.quals.reserve(cap))) return DBGK_ERR_NOMEM;
		s.cap_bytes = cap;
	}
	s.n = n;
	s.total = total;
	if (total) {
		const uint64_t tiles = (total + emitk::kEmitTile - 1) / emitk::kEmitTile;
		const unsigned grid = (unsigned)std::min<uint64_t>(tiles, (uint64_t)n_cu * 64);
		HIPCHK(hipEventRecord(s.ev[2], stream)); // directly in front of the kernel: the copies, the host round trip and an allocation lie before it
		if (s.split_src) { // one launch per plane, both from `seq`, under the one set of offsets
			hipLaunchKernelGGL((emitk::k_emit_gather<false, false>), dim3(grid), dim3(emitk::kEmitBlock), 0, stream, seq, (const uint8_t *)nullptr, s.src,
			                   s.off, (uint32_t)n, total, 0u, reinterpret_cast<uint4 *>(s.bases.p), (uint4 *)nullptr);
			if (with_qual)
				hipLaunchKernelGGL((emitk::k_emit_gather<false, false>), dim3(grid), dim3(emitk::kEmitBlock), 0, stream, seq, (const uint8_t *)nullptr,
				                   s.qsrc, s.off, (uint32_t)n, total, 0u, reinterpret_cast<uint4 *>(s.quals.p), (uint4 *)nullptr);
		} else if (!with_qual && s.lds_one_plane)
			hipLaunchKernelGGL(emitk::k_emit_gather_lds, dim3(grid), dim3(emitk::kEmitBlock), 0, stream, seq, s.src, s.off, (uint32_t)n, total,
			                   reinterpret_cast<uint4 *>(s.bases.p));
		else if (!with_qual) emit_launch_gather<false, false>(s, stream, grid, seq, qual, shift_word);
		else if (subst) emit_launch_gather<true, true>(s, stream, grid, seq, qual, shift_word);
		else emit_launch_gather<true, false>(s, stream, grid, seq, qual, shift_word);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(s.ev[3], stream));
	}
	HIPCHK(hipEventRecord(s.done, stream));
	HIPCHK(hipStreamSynchronize(stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
	*ms_scan = ms;
	*ms_gather = 0; // (stays 0 when nothing is kept: no launch)
	if (total) {
		HIPCHK(hipEventElapsedTime(&ms, s.ev[2], s.ev[3]));
		*ms_gather = ms;
	}
	s.has_qual = with_qual;
	s.have = true;
	return DBGK_OK;
}

// the compact batch to the host; every pointer may be null (quals: only when the batch has a quality plane)
static int emit_results(EmitStage &s, hipStream_t stream, char *bases, char *quals, uint64_t *offsets)
{
	if (bases && s.total) HIPCHK(hipMemcpyAsync(bases, s.bases, s.total, hipMemcpyDeviceToHost, stream));
	if (quals && s.total) HIPCHK(hipMemcpyAsync(quals, s.quals, s.total, hipMemcpyDeviceToHost, stream));
	if (offsets) HIPCHK(hipMemcpyAsync(offsets, s.off, (s.n + 1) * 8, hipMemcpyDeviceToHost, stream));
	HIPCHK(hipStreamSynchronize(stream));
	return DBGK_OK;
}

static void emit_device(const EmitStage &s, const char **d_bases, const char **d_quals, const uint64_t **d_offsets, uint64_t *n_reads, uint64_t *n_bases)
{
	*d_bases = (const char *)s.bases.p;
	if (d_quals) *d_quals = s.has_qual ? (const char *)s.quals.p : nullptr;
	*d_offsets = s.off;
	*n_reads = s.n;
	*n_bases = s.total;
}

// The compact batch of a stage on h's device into h.  launch_batch queues every kernel that reads the pushed pointers on the handle's
// stream (the record engines keep records, the others their table: no engine keeps the pointers), so the event recorded behind the
// push covers every reader and no dbgk_sync is needed for any engine.
static int emit_push(dbgk_handle *h, EmitStage &s)
{
	if (!s.have || h->finalized) return DBGK_ERR_STATE;
	int rc = use_device(h);
	if (rc) return rc;
	HIPCHK(hipStreamWaitEvent(h->stream, s.done, 0));
	// `read` is ONE event: a push into another handle re-records it.  That handle's stream first waits for the earlier record, so
	// the new one lies behind every reader so far, whichever handles they were pushed to.
	if (s.lent) HIPCHK(hipStreamWaitEvent(h->stream, s.read, 0));
	rc = dbgk_push_reads_device(h, (const char *)s.bases.p, s.off, s.n, s.total);
	// (also after a failed push: part of its work may have been queued)
	if (hipEventRecord(s.read, h->stream) == hipSuccess) s.lent = true;
	else if (rc == DBGK_OK) rc = DBGK_ERR_HIP;
	return rc;
}
