// PAIR stage, host side (include/dbgk.h, PAIR section; kernels in dbgk_pair.h): the two mate batches on the device, the split, and
// the two outputs as EmitStage structs, so that their read-back, their device view and their hand-over to a graph handle are
// dbgk_host_emit.h's, with its event ordering.

struct dbgk_pair : StageDev {
	// out[DBGK_PAIR_PAIRED], out[DBGK_PAIR_SINGLE].  Of an EmitStage this stage uses the planes, off, src, len and their capacities,
	// the events and have / has_qual / lent; the counters and the scan's storage of both outputs are out[0]'s.
	EmitStage out[2];
	DevBuf<uint32_t> id[2];   // source id 2 i + mate per output read
	DevBuf<uint32_t> flag[2]; // n + 1 flags: the pair goes to PAIR / to SINGLE
	DevBuf<uint64_t> rank[2]; // their exclusive scans
	uint64_t cap_pairs = 0;
	// dbgk_pair_split_from: the uploaded batches
	DevBuf<uint8_t> in_b[2], in_q[2];
	DevBuf<uint64_t> in_off[2];
	uint64_t in_cap_bytes = 0, in_cap_qual = 0, in_cap_reads = 0;
};

static_assert(DBGK_PAIR_PAIRED == 0 && DBGK_PAIR_SINGLE == 1, "the outputs are indexed by `which`");

extern "C" int dbgk_pair_create(int device, dbgk_pair **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (device < 0) return DBGK_ERR_ARG;
	dbgk_pair *p = new (std::nothrow) dbgk_pair;
	if (!p) return DBGK_ERR_NOMEM;
	int rc = stage_open(*p, device);
	for (int w = 0; !rc && w < 2; ++w) rc = emit_create(p->out[w], pairk::PC_COUNT, false);
	if (rc) {
		dbgk_pair_destroy(p);
		return rc;
	}
	*out = p;
	return DBGK_OK;
}

extern "C" int dbgk_pair_destroy(dbgk_pair *p)
{
	if (!p) return DBGK_ERR_ARG;
	stage_drain(p->device, p->stream);
	for (EmitStage &s : p->out) emit_destroy(s);
	delete p;
	return DBGK_OK;
}

// per-read arrays for n pairs: PAIR holds up to 2 n reads, SINGLE up to n.  (A graph handle that was given an output is waited for.)
static int pair_ensure_reads(dbgk_pair *p, uint64_t n)
{
	if (n <= p->cap_pairs && p->out[0].off) return DBGK_OK;
	for (EmitStage &s : p->out) {
		int rc = emit_reclaim(s, p->stream, true);
		if (rc) return rc;
	}
	p->cap_pairs = 0;
	const uint64_t cap = std::max<uint64_t>(n, 1 << 14);
	for (int w = 0; w < 2; ++w) {
		EmitStage &s = p->out[w];
		const uint64_t reads = w == DBGK_PAIR_PAIRED ? 2 * cap : cap;
		if (s.off.reserve((reads + 1) * 8) || s.len.reserve((reads + 1) * 4) || s.src.reserve(reads * 8) || p->id[w].reserve(reads * 4) ||
		    p->flag[w].reserve((cap + 1) * 4) || p->rank[w].reserve((cap + 1) * 8))
			return DBGK_ERR_NOMEM;
		s.cap_reads = reads;
	}
	p->cap_pairs = cap;
	return DBGK_OK;
}

// the planes of one output for `total` bytes: whole vectors and the room behind the end that the emit planes have
static int pair_ensure_planes(dbgk_pair *p, EmitStage &s, uint64_t total, bool with_qual)
{
	const uint64_t want = ((total + 15) & ~15ull) + 64;
	if (want <= s.cap_bytes && (!with_qual || s.quals)) return DBGK_OK;
	int rc = emit_reclaim(s, p->stream, true);
	if (rc) return rc;
	const bool keep_qual = with_qual || s.quals;
	const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(want, s.cap_bytes), 1 << 20);
	s.cap_bytes = 0;
	if (s.bases.reserve(cap) || (keep_qual && s.quals.reserve(cap))) return DBGK_ERR_NOMEM;
	s.cap_bytes = cap;
	return DBGK_OK;
}

// the split of two batches that lie on the device (the stream is ordered behind whatever wrote them)
static int pair_run(dbgk_pair *p, const uint8_t *b1, const uint8_t *q1, const uint64_t *o1, const uint8_t *b2, const uint8_t *q2, const uint64_t *o2,
                    uint64_t n, dbgk_pair_info *out)
{
	const bool with_qual = q1 != nullptr;
	EmitStage &P = p->out[DBGK_PAIR_PAIRED], &S = p->out[DBGK_PAIR_SINGLE];
	P.have = S.have = false;
	int rc = pair_ensure_reads(p, n);
	if (rc) return rc;
	for (int w = 0; w < 2; ++w) { // the outputs are about to be written: a graph handle that was given one has to be done with it
		rc = emit_reclaim(p->out[w], p->stream, false);
		if (rc) return rc;
	}
	unsigned long long ctr[pairk::PC_COUNT] = {0};
	HIPCHK(hipMemsetAsync(P.ctr, 0, sizeof ctr, p->stream));
	HIPCHK(hipEventRecord(P.ev[0], p->stream));
	const unsigned grid = (unsigned)std::min<uint64_t>((n + emitk::kEmitBlock) / emitk::kEmitBlock, (uint64_t)p->n_cu * 16);
	const uint32_t n32 = (uint32_t)n;
	if (n) {
		hipLaunchKernelGGL(pairk::k_pair_classify, dim3(grid), dim3(emitk::kEmitBlock), 0, p->stream, o1, o2, n32, p->flag[0], p->flag[1], P.ctr);
		HIPCHK(hipGetLastError());
		for (int w = 0; w < 2 && !rc; ++w) rc = stage_scan(P.tmp, p->stream, p->flag[w], p->rank[w], n + 1);
		if (rc) return rc;
		hipLaunchKernelGGL(pairk::k_pair_scatter, dim3(grid), dim3(emitk::kEmitBlock), 0, p->stream, o1, o2, n32, (const uint64_t *)p->rank[0],
		                   (const uint64_t *)p->rank[1], pairk::PairOut{P.len, P.src, p->id[0]}, pairk::PairOut{S.len, S.src, p->id[1]});
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(ctr, P.ctr, sizeof ctr, hipMemcpyDeviceToHost, p->stream));
		HIPCHK(hipStreamSynchronize(p->stream)); // the counts size the scans, the totals the planes
		if (ctr[pairk::PC_BAD]) return DBGK_ERR_ARG; // offsets that decrease, or a read of 2^31 bytes and more
	}
	P.n = ctr[pairk::PC_PAIR_READS], P.total = ctr[pairk::PC_PAIR_BASES];
	S.n = ctr[pairk::PC_SINGLE_READS], S.total = ctr[pairk::PC_SINGLE_BASES];
	for (int w = 0; w < 2; ++w) {
		EmitStage &s = p->out[w];
		if (s.n) rc = stage_scan(P.tmp, p->stream, s.len, s.off, s.n + 1);
		else if (hipMemsetAsync(s.off, 0, 8, p->stream) != hipSuccess) rc = DBGK_ERR_HIP;
		if (rc) return rc;
	}
	HIPCHK(hipEventRecord(P.ev[1], p->stream));
	for (int w = 0; w < 2; ++w) {
		rc = pair_ensure_planes(p, p->out[w], p->out[w].total, with_qual);
		if (rc) return rc;
	}
	const pairk::PairPlanes in{b1, b2, q1, q2};
	HIPCHK(hipEventRecord(P.ev[2], p->stream));
	for (int w = 0; w < 2; ++w) {
		EmitStage &s = p->out[w];
		if (!s.total) continue;
		const uint64_t tiles = (s.total + emitk::kEmitTile - 1) / emitk::kEmitTile;
		const unsigned g = (unsigned)std::min<uint64_t>(tiles, (uint64_t)p->n_cu * 64);
		if (with_qual)
			hipLaunchKernelGGL(pairk::k_pair_gather<true>, dim3(g), dim3(emitk::kEmitBlock), 0, p->stream, in, (const uint64_t *)s.src,
			                   (const uint64_t *)s.off, (uint32_t)s.n, s.total, reinterpret_cast<uint4 *>(s.bases.p), reinterpret_cast<uint4 *>(s.quals.p));
		else
			hipLaunchKernelGGL(pairk::k_pair_gather<false>, dim3(g), dim3(emitk::kEmitBlock), 0, p->stream, in, (const uint64_t *)s.src,
			                   (const uint64_t *)s.off, (uint32_t)s.n, s.total, reinterpret_cast<uint4 *>(s.bases.p), (uint4 *)nullptr);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(P.ev[3], p->stream));
	for (int w = 0; w < 2; ++w) HIPCHK(hipEventRecord(p->out[w].done, p->stream));
	HIPCHK(hipStreamSynchronize(p->stream));
	dbgk_pair_info I{};
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]));
	I.ms_rank = ms;
	HIPCHK(hipEventElapsedTime(&ms, P.ev[2], P.ev[3]));
	I.ms_gather = (P.total || S.total) ? ms : 0; // (0 when nothing is kept: no launch)
	I.n_pairs_in = n;
	I.pair_reads = P.n, I.pair_bases = P.total, I.single_reads = S.n, I.single_bases = S.total;
	I.max_len = ctr[pairk::PC_MAX_LEN];
	for (int w = 0; w < 2; ++w) {
		p->out[w].has_qual = with_qual;
		p->out[w].have = true;
	}
	*out = I;
	return DBGK_OK;
}

// a plane handed in from outside: 16-byte aligned, and not one of the stage's own output planes
static bool pair_device_plane_ok(const dbgk_pair *p, const char *ptr)
{
	if ((uintptr_t)ptr & 15u) return false;
	const uint8_t *u = (const uint8_t *)ptr;
	for (int w = 0; w < 2; ++w)
		for (const uint8_t *own : {p->out[w].bases.p, p->out[w].quals.p})
			if (u && own && u >= own && u < own + p->out[w].cap_bytes) return false;
	return true;
}

extern "C" int dbgk_pair_split_device(dbgk_pair *p, const char *d_bases1, const char *d_quals1, const uint64_t *d_offsets1, const char *d_bases2,
                                      const char *d_quals2, const uint64_t *d_offsets2, uint64_t n, dbgk_pair_info *out)
{
	if (!p || !out || n >= (1ull << 31) || (d_quals1 == nullptr) != (d_quals2 == nullptr)) return DBGK_ERR_ARG;
	if (n && (!d_offsets1 || !d_offsets2 || ((uintptr_t)d_offsets1 & 7u) || ((uintptr_t)d_offsets2 & 7u))) return DBGK_ERR_ARG;
	for (const char *plane : {d_bases1, d_quals1, d_bases2, d_quals2})
		if (!pair_device_plane_ok(p, plane)) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(p->device));
	return pair_run(p, (const uint8_t *)d_bases1, (const uint8_t *)d_quals1, d_offsets1, (const uint8_t *)d_bases2, (const uint8_t *)d_quals2, d_offsets2,
	                n, out);
}

extern "C" int dbgk_pair_split_from(dbgk_pair *p, const char *bases1, const char *quals1, const uint64_t *offsets1, const char *bases2,
                                    const char *quals2, const uint64_t *offsets2, uint64_t n, dbgk_pair_info *out)
{
	if (!p || !out || !offsets1 || !offsets2 || n >= (1ull << 31) || (quals1 == nullptr) != (quals2 == nullptr)) return DBGK_ERR_ARG;
	const char *bases[2] = {bases1, bases2}, *quals[2] = {quals1, quals2};
	const uint64_t *offsets[2] = {offsets1, offsets2};
	uint64_t most = 0;
	for (int w = 0; w < 2; ++w) {
		if (offsets[w][0] != 0) return DBGK_ERR_ARG;
		for (uint64_t i = 0; i < n; ++i)
			if (offsets[w][i + 1] < offsets[w][i] || offsets[w][i + 1] - offsets[w][i] >= (1ull << 31)) return DBGK_ERR_ARG;
		if (offsets[w][n] && (!bases[w] || (quals1 && !quals[w]))) return DBGK_ERR_ARG;
		most = std::max(most, offsets[w][n]);
	}
	const bool with_qual = quals1 != nullptr;
	p->out[0].have = p->out[1].have = false;
	HIPCHK(hipSetDevice(p->device));
	if (most + 16 > p->in_cap_bytes || n > p->in_cap_reads || !p->in_off[0] || (with_qual && p->in_cap_qual < p->in_cap_bytes)) {
		HIPCHK(hipStreamSynchronize(p->stream));
		const uint64_t bytes = std::max<uint64_t>(std::max<uint64_t>(most + 16, p->in_cap_bytes), 1 << 20);
		const uint64_t reads = std::max<uint64_t>(std::max<uint64_t>(n, p->in_cap_reads), 1 << 14);
		const bool qual = with_qual || p->in_cap_qual;
		p->in_cap_bytes = p->in_cap_qual = p->in_cap_reads = 0;
		for (int w = 0; w < 2; ++w)
			if (p->in_b[w].reserve(bytes) || (qual && p->in_q[w].reserve(bytes)) || p->in_off[w].reserve((reads + 1) * 8)) return DBGK_ERR_NOMEM;
		p->in_cap_bytes = bytes;
		p->in_cap_qual = qual ? bytes : 0;
		p->in_cap_reads = reads;
	}
	for (int w = 0; w < 2; ++w) {
		const uint64_t nb = offsets[w][n];
		if (nb) HIPCHK(hipMemcpyAsync(p->in_b[w], bases[w], nb, hipMemcpyHostToDevice, p->stream));
		if (nb && with_qual) HIPCHK(hipMemcpyAsync(p->in_q[w], quals[w], nb, hipMemcpyHostToDevice, p->stream));
		HIPCHK(hipMemcpyAsync(p->in_off[w], offsets[w], (n + 1) * 8, hipMemcpyHostToDevice, p->stream));
	}
	HIPCHK(hipStreamSynchronize(p->stream)); // the caller's buffers are free on return
	return pair_run(p, p->in_b[0], with_qual ? p->in_q[0].p : nullptr, p->in_off[0], p->in_b[1], with_qual ? p->in_q[1].p : nullptr, p->in_off[1], n, out);
}

extern "C" int dbgk_pair_results(dbgk_pair *p, int which, char *bases, char *quals, uint64_t *offsets, uint32_t *src_ids)
{
	if (!p || (which != DBGK_PAIR_PAIRED && which != DBGK_PAIR_SINGLE)) return DBGK_ERR_ARG;
	EmitStage &s = p->out[which];
	if (!s.have) return DBGK_ERR_STATE;
	if (quals && !s.has_qual) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(p->device));
	if (src_ids && s.n) HIPCHK(hipMemcpyAsync(src_ids, p->id[which], s.n * 4, hipMemcpyDeviceToHost, p->stream));
	return emit_results(s, p->stream, bases, quals, offsets);
}

extern "C" int dbgk_pair_device(dbgk_pair *p, int which, const char **d_bases, const char **d_quals, const uint64_t **d_offsets, uint64_t *n_reads,
                                uint64_t *n_bases)
{
	if (!p || (which != DBGK_PAIR_PAIRED && which != DBGK_PAIR_SINGLE) || !d_bases || !d_quals || !d_offsets || !n_reads || !n_bases)
		return DBGK_ERR_ARG;
	if (!p->out[which].have) return DBGK_ERR_STATE;
	emit_device(p->out[which], d_bases, d_quals, d_offsets, n_reads, n_bases);
	return DBGK_OK;
}

extern "C" int dbgk_push_pairs(dbgk_handle *h, dbgk_pair *p, int which)
{
	if (!h || !p || (which != DBGK_PAIR_PAIRED && which != DBGK_PAIR_SINGLE)) return DBGK_ERR_ARG;
	if (h->device != p->device) return DBGK_ERR_ARG;
	return emit_push(h, p->out[which]);
}
