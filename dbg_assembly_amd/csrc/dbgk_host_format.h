// FORMAT stage, host side (include/dbgk.h, FORMAT section; kernels in dbgk_format.h): the output text of one batch on the device,
// its read-back and its device view.  The launches of a call follow each other on one stream; the host reads the counters and the
// total in between, which size the text.  The suffix plane comes from the host (checked there, uploaded) or lies on the device
// (checked there by k_annot_check of dbgk_annot.h); fmt_run is the same for both.

struct dbgk_fmt : StageDev {
	int format = 1;
	uint32_t marker = 0;
	DevBuf<uint8_t> out; // 16-byte vectors, the pad of the last one 0, 64 readable bytes behind
	uint64_t n_out = 0;
	bool have = false;
	DevBuf<uint32_t> len; // n + 1 output lengths and their exclusive scan
	DevBuf<uint64_t> coff;
	uint64_t cap_recs = 0;
	ScanTmp tmp; // the scan's temporary storage
	DevBuf<unsigned long long> ctr;
	DevBuf<uint8_t> suf; // the uploaded suffix plane
	DevBuf<uint64_t> soff;
	DevBuf<uint32_t> suf_bad; // what k_annot_check found in the offsets of a suffix plane on the device
	// dbgk_fmt_records: the uploaded batch
	DevBuf<uint8_t> in_text, in_b, in_q;
	DevBuf<uint64_t> in_off;
	DevBuf<dbgk_parse_rec> in_rec;
	uint64_t in_cap_recs = 0;
	StageEvents<4> ev; // length + scan: [0] .. [1]; gather: [2] .. [3]
};

extern "C" int dbgk_fmt_create(int32_t format, int32_t marker, int device, dbgk_fmt **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (device < 0 || (format != 1 && format != 2) || marker < 0 || marker > 255) return DBGK_ERR_ARG;
	dbgk_fmt *f = new (std::nothrow) dbgk_fmt;
	if (!f) return DBGK_ERR_NOMEM;
	f->format = format;
	f->marker = (uint32_t)marker;
	int rc = stage_open(*f, device);
	if (!rc) rc = f->ev.create();
	if (!rc) rc = f->ctr.reserve(fmtk::FC_COUNT * sizeof(unsigned long long));
	if (rc) {
		dbgk_fmt_destroy(f);
		return rc;
	}
	*out = f;
	return DBGK_OK;
}

extern "C" int dbgk_fmt_destroy(dbgk_fmt *f)
{
	if (!f) return DBGK_ERR_ARG;
	stage_drain(f->device, f->stream);
	delete f;
	return DBGK_OK;
}

// The suffix plane of a call as the kernels read it: both null for all empty (a plane of empty suffixes is no plane).
struct FmtSuffix {
	const uint8_t *suf = nullptr;
	const uint64_t *soff = nullptr;
};

// a plane on the host: checked here, uploaded on the stream
static int fmt_suffix_from_host(dbgk_fmt *f, uint64_t n, const char *suffix, const uint64_t *suffix_offsets, FmtSuffix &S)
{
	f->have = false;
	uint64_t n_suf = 0;
	if (suffix_offsets && n) {
		if (suffix_offsets[0] != 0) return DBGK_ERR_ARG;
		for (uint64_t i = 0; i < n; ++i)
			if (suffix_offsets[i + 1] < suffix_offsets[i]) return DBGK_ERR_ARG;
		n_suf = suffix_offsets[n];
		if (n_suf >= (1ull << 32) || (n_suf && !suffix)) return DBGK_ERR_ARG;
	}
	HIPCHK(hipStreamSynchronize(f->stream));
	if (n_suf) {
		if (f->suf.reserve(n_suf + 16, 1 << 16) || f->soff.reserve((n + 1) * 8, 1 << 17)) return DBGK_ERR_NOMEM;
		HIPCHK(hipMemcpyAsync(f->suf, suffix, n_suf, hipMemcpyHostToDevice, f->stream));
		HIPCHK(hipMemcpyAsync(f->soff, suffix_offsets, (n + 1) * 8, hipMemcpyHostToDevice, f->stream));
		S.suf = f->suf;
		S.soff = f->soff;
	}
	return DBGK_OK;
}

// a plane on the device: the same checks by k_annot_check (dbgk_annot.h), answered before a byte of the plane is read
static int fmt_suffix_on_device(dbgk_fmt *f, uint64_t n, const uint8_t *d_suffix, const uint64_t *d_suffix_offsets, FmtSuffix &S)
{
	f->have = false;
	if (!d_suffix_offsets || !n) return DBGK_OK;
	HIPCHK(hipStreamSynchronize(f->stream));
	if (f->suf_bad.reserve(sizeof(uint32_t))) return DBGK_ERR_NOMEM;
	HIPCHK(hipMemsetAsync(f->suf_bad, 0, sizeof(uint32_t), f->stream));
	const unsigned grid = (unsigned)std::min<uint64_t>((n + emitk::kEmitBlock - 1) / emitk::kEmitBlock, (uint64_t)f->n_cu * 16);
	hipLaunchKernelGGL(annotk::k_annot_check, dim3(grid), dim3(emitk::kEmitBlock), 0, f->stream, d_suffix_offsets, (uint32_t)n, f->suf_bad.p);
	HIPCHK(hipGetLastError());
	uint32_t bad = 0;
	uint64_t n_suf = 0;
	HIPCHK(hipMemcpyAsync(&bad, f->suf_bad, sizeof bad, hipMemcpyDeviceToHost, f->stream));
	HIPCHK(hipMemcpyAsync(&n_suf, d_suffix_offsets + n, 8, hipMemcpyDeviceToHost, f->stream));
	HIPCHK(hipStreamSynchronize(f->stream));
	if (bad || (n_suf && !d_suffix)) return DBGK_ERR_ARG;
	if (n_suf) {
		S.suf = d_suffix;
		S.soff = d_suffix_offsets;
	}
	return DBGK_OK;
}

// n records that lie on the device (the stream is ordered behind whatever wrote them), and their suffix plane, checked by one of
// the two functions above
static int fmt_run(dbgk_fmt *f, const uint8_t *text, uint64_t n_text, const dbgk_parse_rec *recs, const uint8_t *bases, const uint8_t *quals,
                   const uint64_t *off, uint64_t n, const FmtSuffix &S, dbgk_fmt_info *out)
{
	f->have = false;
	const bool fastq = f->format == 1;
	HIPCHK(hipStreamSynchronize(f->stream));
	if (n + 1 > f->cap_recs || !f->len || !f->coff) {
		const uint64_t cap = std::max<uint64_t>(n + 1, 1 << 14);
		f->cap_recs = 0;
		if (f->len.reserve(cap * 4) || f->coff.reserve(cap * 8)) return DBGK_ERR_NOMEM;
		f->cap_recs = cap;
	}
	if (n) {
		const int rc = stage_scan_reserve(f->tmp, f->stream, f->len, f->coff, n + 1);
		if (rc) return rc;
	}
	const fmtk::FmtIn in{text, recs, bases, quals, off, S.suf, S.soff};
	unsigned long long ctr[fmtk::FC_COUNT] = {0};
	uint64_t total = 0;
	HIPCHK(hipEventRecord(f->ev[0], f->stream));
	if (n) {
		HIPCHK(hipMemsetAsync(f->ctr, 0, sizeof ctr, f->stream));
		const unsigned grid = (unsigned)std::min<uint64_t>((n + emitk::kEmitBlock) / emitk::kEmitBlock, (uint64_t)f->n_cu * 16);
		hipLaunchKernelGGL(fmtk::k_fmt_len, dim3(grid), dim3(emitk::kEmitBlock), 0, f->stream, in, (uint32_t)n, (uint32_t)n_text, (uint32_t)fastq, f->len,
		                   f->ctr);
		HIPCHK(hipGetLastError());
		const int rc = stage_scan(f->tmp, f->stream, f->len, f->coff, n + 1);
		if (rc) return rc;
	}
	HIPCHK(hipEventRecord(f->ev[1], f->stream));
	if (n) {
		HIPCHK(hipMemcpyAsync(&total, f->coff + n, 8, hipMemcpyDeviceToHost, f->stream));
		HIPCHK(hipMemcpyAsync(ctr, f->ctr, sizeof ctr, hipMemcpyDeviceToHost, f->stream));
	}
	HIPCHK(hipStreamSynchronize(f->stream)); // the total sizes the text; the caller's suffix plane is free from here on
	if (ctr[fmtk::FC_BAD]) return DBGK_ERR_ARG; // a header that leaves the text, offsets that decrease, a record of 2^32 bytes
	// whole vectors, and room behind the end for the 16-byte reads of the kernels that take the text as their input
	if (f->out.reserve(((total + 15) & ~15ull) + 64, 1 << 20)) return DBGK_ERR_NOMEM;
	if (total) {
		const uint64_t tiles = (total + emitk::kEmitTile - 1) / emitk::kEmitTile;
		const unsigned grid = (unsigned)std::min<uint64_t>(tiles, (uint64_t)f->n_cu * 64);
		HIPCHK(hipEventRecord(f->ev[2], f->stream));
		if (fastq)
			hipLaunchKernelGGL(fmtk::k_fmt_gather<true>, dim3(grid), dim3(emitk::kEmitBlock), 0, f->stream, in, (const uint64_t *)f->coff, (uint32_t)n, total,
			                   f->marker, reinterpret_cast<uint4 *>(f->out.p));
		else
			hipLaunchKernelGGL(fmtk::k_fmt_gather<false>, dim3(grid), dim3(emitk::kEmitBlock), 0, f->stream, in, (const uint64_t *)f->coff, (uint32_t)n, total,
			                   f->marker, reinterpret_cast<uint4 *>(f->out.p));
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(f->ev[3], f->stream));
		HIPCHK(hipStreamSynchronize(f->stream));
	}
	dbgk_fmt_info I{};
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, f->ev[0], f->ev[1]));
	I.ms_scan = ms;
	if (total) {
		HIPCHK(hipEventElapsedTime(&ms, f->ev[2], f->ev[3]));
		I.ms_gather = ms;
	}
	I.n_records = n;
	I.out_bytes = total;
	I.head_bytes = ctr[fmtk::FC_HEAD], I.suffix_bytes = ctr[fmtk::FC_SUFFIX], I.seq_bytes = ctr[fmtk::FC_SEQ];
	f->n_out = total;
	f->have = true;
	*out = I;
	return DBGK_OK;
}

// the arguments both calls share
static bool fmt_args_ok(const dbgk_fmt *f, const void *text, uint64_t n_text, const void *recs, const void *bases, const void *quals,
                        const void *offsets, uint64_t n, const dbgk_fmt_info *out)
{
	if (!f || !out || n >= (1ull << 31) || n_text >= (1ull << 31) || (n_text && !text)) return false;
	if ((f->format == 1) != (quals != nullptr)) return false; // FASTQ has a quality plane, FASTA has none
	if (n && (!recs || !offsets || !bases)) return false;
	return true;
}

// what both device entries ask of the batch: alignment, and none of the planes (the suffix plane included) the text about to be written
static bool fmt_device_args_ok(const dbgk_fmt *f, const char *d_text, const dbgk_parse_rec *d_recs, const char *d_bases, const char *d_quals,
                               const uint64_t *d_offsets, const char *d_suffix)
{
	if (((uintptr_t)d_text & 15u) || ((uintptr_t)d_bases & 15u) || ((uintptr_t)d_quals & 15u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_recs & 3u))
		return false;
	for (const char *p : {d_text, d_bases, d_quals, d_suffix}) {
		const uint8_t *u = (const uint8_t *)p;
		if (u && f->out && u >= f->out && u < f->out + f->out.cap) return false;
	}
	return true;
}

extern "C" int dbgk_fmt_records_device(dbgk_fmt *f, const char *d_text, uint64_t n_text, const dbgk_parse_rec *d_recs, const char *d_bases,
                                       const char *d_quals, const uint64_t *d_offsets, uint64_t n, const char *suffix,
                                       const uint64_t *suffix_offsets, dbgk_fmt_info *out)
{
	if (!fmt_args_ok(f, d_text, n_text, d_recs, d_bases, d_quals, d_offsets, n, out)) return DBGK_ERR_ARG;
	if (!fmt_device_args_ok(f, d_text, d_recs, d_bases, d_quals, d_offsets, nullptr)) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(f->device));
	FmtSuffix S;
	const int rc = fmt_suffix_from_host(f, n, suffix, suffix_offsets, S);
	if (rc) return rc;
	return fmt_run(f, (const uint8_t *)d_text, n_text, d_recs, (const uint8_t *)d_bases, (const uint8_t *)d_quals, d_offsets, n, S, out);
}

extern "C" int dbgk_fmt_records_device_suffix(dbgk_fmt *f, const char *d_text, uint64_t n_text, const dbgk_parse_rec *d_recs, const char *d_bases,
                                              const char *d_quals, const uint64_t *d_offsets, uint64_t n, const char *d_suffix,
                                              const uint64_t *d_suffix_offsets, dbgk_fmt_info *out)
{
	if (!fmt_args_ok(f, d_text, n_text, d_recs, d_bases, d_quals, d_offsets, n, out)) return DBGK_ERR_ARG;
	if (!fmt_device_args_ok(f, d_text, d_recs, d_bases, d_quals, d_offsets, d_suffix)) return DBGK_ERR_ARG;
	if (((uintptr_t)d_suffix & 15u) || ((uintptr_t)d_suffix_offsets & 7u)) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(f->device));
	FmtSuffix S;
	const int rc = fmt_suffix_on_device(f, n, (const uint8_t *)d_suffix, d_suffix_offsets, S);
	if (rc) return rc;
	return fmt_run(f, (const uint8_t *)d_text, n_text, d_recs, (const uint8_t *)d_bases, (const uint8_t *)d_quals, d_offsets, n, S, out);
}

extern "C" int dbgk_fmt_records(dbgk_fmt *f, const char *text, uint64_t n_text, const dbgk_parse_rec *recs, const char *bases, const char *quals,
                                const uint64_t *offsets, uint64_t n, const char *suffix, const uint64_t *suffix_offsets, dbgk_fmt_info *out)
{
	if (!fmt_args_ok(f, text, n_text, recs, bases, quals, offsets, n, out)) return DBGK_ERR_ARG;
	f->have = false;
	uint64_t nb = 0;
	if (n) {
		for (uint64_t i = 0; i < n; ++i) // (the planes are uploaded up to offsets[n])
			if (offsets[i + 1] < offsets[i]) return DBGK_ERR_ARG;
		nb = offsets[n];
	}
	HIPCHK(hipSetDevice(f->device));
	HIPCHK(hipStreamSynchronize(f->stream));
	if (n + 1 > f->in_cap_recs || !f->in_off || !f->in_rec) {
		const uint64_t cap = std::max<uint64_t>(n + 1, 1 << 14);
		f->in_cap_recs = 0;
		if (f->in_off.reserve(cap * 8) || f->in_rec.reserve(cap * sizeof(dbgk_parse_rec))) return DBGK_ERR_NOMEM;
		f->in_cap_recs = cap;
	}
	if (f->in_text.reserve(n_text + 16, 1 << 20) || f->in_b.reserve(nb + 16, 1 << 20) || (quals && f->in_q.reserve(nb + 16, 1 << 20)))
		return DBGK_ERR_NOMEM;
	if (n_text) HIPCHK(hipMemcpyAsync(f->in_text, text, n_text, hipMemcpyHostToDevice, f->stream));
	if (nb) HIPCHK(hipMemcpyAsync(f->in_b, bases, nb, hipMemcpyHostToDevice, f->stream));
	if (nb && quals) HIPCHK(hipMemcpyAsync(f->in_q, quals, nb, hipMemcpyHostToDevice, f->stream));
	if (n) {
		HIPCHK(hipMemcpyAsync(f->in_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, f->stream));
		HIPCHK(hipMemcpyAsync(f->in_rec, recs, n * sizeof(dbgk_parse_rec), hipMemcpyHostToDevice, f->stream));
	}
	HIPCHK(hipStreamSynchronize(f->stream)); // the caller's buffers are free on return
	FmtSuffix S;
	const int rc = fmt_suffix_from_host(f, n, suffix, suffix_offsets, S);
	if (rc) return rc;
	return fmt_run(f, f->in_text, n_text, f->in_rec, f->in_b, quals ? f->in_q.p : nullptr, f->in_off, n, S, out);
}

extern "C" int dbgk_fmt_results(dbgk_fmt *f, void *out, uint64_t capacity)
{
	if (!f) return DBGK_ERR_ARG;
	if (!f->have) return DBGK_ERR_STATE;
	if (capacity < f->n_out || (f->n_out && !out)) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(f->device));
	if (f->n_out) HIPCHK(hipMemcpyAsync(out, f->out, f->n_out, hipMemcpyDeviceToHost, f->stream));
	HIPCHK(hipStreamSynchronize(f->stream));
	return DBGK_OK;
}

extern "C" int dbgk_fmt_device(dbgk_fmt *f, const void **d_out, uint64_t *n_out)
{
	if (!f || !d_out || !n_out) return DBGK_ERR_ARG;
	if (!f->have) return DBGK_ERR_STATE;
	*d_out = f->out.p;
	*n_out = f->n_out;
	return DBGK_OK;
}

extern "C" int dbgk_parse_recs_device(dbgk_parse *p, const dbgk_parse_rec **d_recs)
{
	if (!p || !d_recs) return DBGK_ERR_ARG;
	if (!p->out.have) return DBGK_ERR_STATE;
	*d_recs = p->rec.p;
	return DBGK_OK;
}

extern "C" int dbgk_parse_text_device(dbgk_parse *p, const char **d_text, uint64_t *n_bytes)
{
	if (!p || !d_text || !n_bytes) return DBGK_ERR_ARG;
	if (!p->out.have) return DBGK_ERR_STATE;
	*d_text = (const char *)p->last_text;
	*n_bytes = p->last_n;
	return DBGK_OK;
}
