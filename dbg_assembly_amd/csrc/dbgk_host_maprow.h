// ROWS stage, host side (include/dbgk.h, ROWS section; kernels in dbgk_maprow.h): the three output streams of one batch on the device,
// their read-back and their device views.  The launches of a call follow each other on one stream; the host reads the counters and
// the three totals in between, which decide whether any text is written and size it.

struct dbgk_maprow : StageDev {
	int mode = DBGK_MAPROW_READS;
	uint64_t dlo = 0, dhi = 0; // the delimiter set: bit c of dlo for a byte c < 64, bit c - 64 of dhi for 64 <= c < 128
	uint32_t min_len = 0;
	// the contig table
	DevBuf<uint8_t> names;
	DevBuf<uint64_t> name_off;
	DevBuf<uint32_t> ctg_len;
	uint64_t n_contigs = 0;
	bool have_contigs = false;
	// per side: the hits taken from a mapper (or uploaded), the token spans, and the batch dbgk_maprow_rows uploads
	struct Side {
		DevBuf<dbgk_map_hit> hits; // 2 n_hits hits
		uint64_t n_hits = 0;
		bool have_hits = false;
		DevBuf<uint4> ids;
		DevBuf<uint8_t> in_text, in_b;
		DevBuf<uint64_t> in_off;
		DevBuf<dbgk_parse_rec> in_rec;
	} side[2];
	DevBuf<uint32_t> len[DBGK_MAPROW_STREAMS]; // n + 1 lengths per stream and their exclusive scans
	DevBuf<uint64_t> coff[DBGK_MAPROW_STREAMS];
	DevBuf<uint32_t> cls;
	uint64_t cap_items = 0;
	DevBuf<uint8_t> plane; // the numeric segments: 2 n slots of rowk::kSlot bytes
	DevBuf<uint8_t> out[DBGK_MAPROW_STREAMS]; // 16-byte vectors, the pad of the last one 0, 64 readable bytes behind
	uint64_t n_out[DBGK_MAPROW_STREAMS] = {0, 0, 0};
	bool have = false;
	ScanTmp tmp;
	DevBuf<unsigned long long> ctr;
	DevBuf<uint32_t> bad;
	StageEvents<6> ev; // lengths + scans: [0] .. [1]; segments + write: [2] .. [3]; take_hits: [4] on the mapper's stream, [5] on this one
};

extern "C" int dbgk_maprow_create(int32_t mode, const char *format_delims, int32_t min_read_len, int device, dbgk_maprow **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (device < 0 || (mode != DBGK_MAPROW_READS && mode != DBGK_MAPROW_PAIR) || !format_delims || min_read_len < 0) return DBGK_ERR_ARG;
	const size_t nd = strnlen(format_delims, 17);
	if (nd < 1 || nd > 16) return DBGK_ERR_ARG;
	uint64_t dlo = 0, dhi = 0;
	for (size_t k = 0; k < nd; ++k) {
		const unsigned c = (unsigned char)format_delims[k];
		if (c >= 128u) return DBGK_ERR_ARG;
		(c < 64u ? dlo : dhi) |= 1ull << (c & 63u);
	}
	dbgk_maprow *r = new (std::nothrow) dbgk_maprow;
	if (!r) return DBGK_ERR_NOMEM;
	r->mode = mode;
	r->dlo = dlo;
	r->dhi = dhi;
	r->min_len = (uint32_t)min_read_len;
	int rc = stage_open(*r, device);
	if (!rc) rc = r->ev.create();
	if (!rc) rc = r->ctr.reserve(rowk::RC_COUNT * sizeof(unsigned long long));
	if (!rc) rc = r->bad.reserve(sizeof(uint32_t));
	if (rc) {
		dbgk_maprow_destroy(r);
		return rc;
	}
	*out = r;
	return DBGK_OK;
}

extern "C" int dbgk_maprow_destroy(dbgk_maprow *r)
{
	if (!r) return DBGK_ERR_ARG;
	stage_drain(r->device, r->stream);
	delete r;
	return DBGK_OK;
}

extern "C" int dbgk_maprow_set_contigs(dbgk_maprow *r, const char *names, const uint64_t *name_offsets, const uint32_t *lengths, uint64_t n)
{
	if (!r || !name_offsets || name_offsets[0] != 0 || n >= (1ull << 31) || (n && !lengths)) return DBGK_ERR_ARG;
	for (uint64_t i = 0; i < n; ++i)
		if (name_offsets[i + 1] < name_offsets[i]) return DBGK_ERR_ARG;
	const uint64_t total = name_offsets[n];
	if (total && !names) return DBGK_ERR_ARG;
	r->have_contigs = false;
	r->have = false;
	HIPCHK(hipSetDevice(r->device));
	HIPCHK(hipStreamSynchronize(r->stream));
	if (r->names.reserve(total + 16) || r->name_off.reserve((n + 1) * 8) || r->ctg_len.reserve(std::max<uint64_t>(n, 1) * 4)) return DBGK_ERR_NOMEM;
	if (total) HIPCHK(hipMemcpyAsync(r->names, names, total, hipMemcpyHostToDevice, r->stream));
	HIPCHK(hipMemcpyAsync(r->name_off, name_offsets, (n + 1) * 8, hipMemcpyHostToDevice, r->stream));
	if (n) HIPCHK(hipMemcpyAsync(r->ctg_len, lengths, n * 4, hipMemcpyHostToDevice, r->stream));
	HIPCHK(hipStreamSynchronize(r->stream));
	r->n_contigs = n;
	r->have_contigs = true;
	return DBGK_OK;
}

// room for the 2 n hits of a side
static int maprow_hits_reserve(dbgk_maprow *r, int side, uint64_t n)
{
	dbgk_maprow::Side &S = r->side[side];
	S.have_hits = false;
	return S.hits.reserve((2 * n + 1) * sizeof(dbgk_map_hit), (1 << 15) * sizeof(dbgk_map_hit));
}

extern "C" int dbgk_maprow_take_hits(dbgk_maprow *r, int32_t side, dbgk_map *m)
{
	if (!r || !m || (side != 0 && side != 1) || r->device != m->device) return DBGK_ERR_ARG;
	if (!m->have_hits) return DBGK_ERR_STATE;
	const uint64_t n = m->last.reads;
	HIPCHK(hipSetDevice(r->device));
	HIPCHK(hipStreamSynchronize(r->stream)); // nothing queued reads the side's old buffer
	if (maprow_hits_reserve(r, side, n)) return DBGK_ERR_NOMEM;
	dbgk_maprow::Side &S = r->side[side];
	if (n) {
		// behind the mapper's batch, and the mapper's next batch behind the copy
		HIPCHK(hipEventRecord(r->ev[4], m->stream));
		HIPCHK(hipStreamWaitEvent(r->stream, r->ev[4], 0));
		HIPCHK(hipMemcpyAsync(S.hits, m->d_hits, 2 * n * sizeof(dbgk_map_hit), hipMemcpyDeviceToDevice, r->stream));
		HIPCHK(hipEventRecord(r->ev[5], r->stream));
		HIPCHK(hipStreamWaitEvent(m->stream, r->ev[5], 0));
	}
	S.n_hits = n;
	S.have_hits = true;
	return DBGK_OK;
}

// n items whose sides lie on the device (the stream is ordered behind whatever wrote them); the hits are in r->side[]
static int maprow_run(dbgk_maprow *r, const dbgk_maprow_side *sides, uint64_t n, dbgk_maprow_info *out)
{
	r->have = false;
	const bool pair = r->mode == DBGK_MAPROW_PAIR;
	const int n_sides = pair ? 2 : 1;
	HIPCHK(hipStreamSynchronize(r->stream));
	if (n + 1 > r->cap_items || !r->cls) {
		const uint64_t cap = std::max<uint64_t>(n + 1, 1 << 14);
		r->cap_items = 0;
		for (int s = 0; s < DBGK_MAPROW_STREAMS; ++s)
			if (r->len[s].reserve(cap * 4) || r->coff[s].reserve(cap * 8)) return DBGK_ERR_NOMEM;
		if (r->cls.reserve(cap * 4) || r->side[0].ids.reserve(cap * sizeof(uint4)) || r->side[1].ids.reserve(cap * sizeof(uint4))) return DBGK_ERR_NOMEM;
		r->cap_items = cap;
	}
	if (n) {
		const int rc = stage_scan_reserve(r->tmp, r->stream, r->len[0], r->coff[0], n + 1);
		if (rc) return rc;
	}
	rowk::RowIn in{};
	for (int s = 0; s < 2; ++s) {
		const dbgk_maprow_side &H = sides[pair ? s : 0];
		// READS: side 1 is side 0 with its hits one further on, so slot j of item i is hits[2 i] of side j in both modes
		in.s[s] = rowk::RowSide{(const uint8_t *)H.text,     H.recs, (const uint8_t *)H.bases, H.offsets, r->side[pair ? s : 0].hits.p + (pair ? 0 : s),
		                        r->side[pair ? s : 0].ids.p};
	}
	in.names = r->names;
	in.name_off = r->name_off;
	in.ctg_len = r->ctg_len;
	in.n_contigs = (uint32_t)r->n_contigs;
	in.pair = pair ? 1u : 0u;
	in.min_len = r->min_len;
	unsigned long long ctr[rowk::RC_COUNT] = {0};
	uint64_t total[DBGK_MAPROW_STREAMS] = {0, 0, 0};
	uint32_t bad = 0;
	HIPCHK(hipEventRecord(r->ev[0], r->stream));
	if (n) {
		HIPCHK(hipMemsetAsync(r->ctr, 0, sizeof ctr, r->stream));
		HIPCHK(hipMemsetAsync(r->bad, 0, sizeof bad, r->stream));
		const unsigned grid = (unsigned)std::min<uint64_t>((n + emitk::kEmitBlock) / emitk::kEmitBlock, (uint64_t)r->n_cu * 16);
		for (int s = 0; s < n_sides; ++s) {
			const rowk::IdsIn ids{(const uint8_t *)sides[s].text, sides[s].recs, r->side[s].ids.p, r->bad.p};
			hipLaunchKernelGGL(rowk::k_maprow_ids, dim3(grid), dim3(emitk::kEmitBlock), 0, r->stream, ids, (uint32_t)n, (uint32_t)sides[s].n_text, r->dlo, r->dhi);
			HIPCHK(hipGetLastError());
		}
		HIPCHK(hipMemcpyAsync(&bad, r->bad, sizeof bad, hipMemcpyDeviceToHost, r->stream));
		HIPCHK(hipStreamSynchronize(r->stream));
		if (bad) return DBGK_ERR_ARG; // a header that leaves the text: no token span of it is read
		hipLaunchKernelGGL(rowk::k_maprow_len, dim3(grid), dim3(emitk::kEmitBlock), 0, r->stream, in, (uint32_t)n, r->len[0].p, r->len[1].p, r->len[2].p, r->cls.p,
		                   r->ctr.p);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(ctr, r->ctr, sizeof ctr, hipMemcpyDeviceToHost, r->stream));
		HIPCHK(hipStreamSynchronize(r->stream));
		if (ctr[rowk::RC_BAD]) return DBGK_ERR_ARG; // a hit no row can be made of, offsets that decrease, a line of 2^32 bytes
		if (!ctr[rowk::RC_UNPRINTABLE]) {
			for (int s = 0; s < DBGK_MAPROW_STREAMS; ++s) {
				const int rc = stage_scan(r->tmp, r->stream, r->len[s], r->coff[s], n + 1);
				if (rc) return rc;
				HIPCHK(hipMemcpyAsync(&total[s], r->coff[s] + n, 8, hipMemcpyDeviceToHost, r->stream));
			}
		}
	}
	HIPCHK(hipEventRecord(r->ev[1], r->stream));
	HIPCHK(hipStreamSynchronize(r->stream)); // the totals size the streams
	for (int s = 0; s < DBGK_MAPROW_STREAMS; ++s)
		if (r->out[s].reserve(((total[s] + 15) & ~15ull) + 64, 1 << 16)) return DBGK_ERR_NOMEM;
	const bool any = total[0] || total[1] || total[2];
	if (any) {
		const bool rows = total[0] || total[1] || (pair && total[2]);
		if (rows && r->plane.reserve(2 * n * rowk::kSlot, 1 << 20)) return DBGK_ERR_NOMEM;
		HIPCHK(hipEventRecord(r->ev[2], r->stream));
		if (rows) {
			const uint64_t groups = (2 * n + emitk::kEmitBlock - 1) / emitk::kEmitBlock;
			hipLaunchKernelGGL(rowk::k_maprow_num, dim3((unsigned)std::min<uint64_t>(groups, (uint64_t)r->n_cu * 5)), dim3(emitk::kEmitBlock), 0, r->stream, in,
			                   (const uint32_t *)r->cls.p, (uint32_t)n, reinterpret_cast<uint4 *>(r->plane.p));
			HIPCHK(hipGetLastError());
		}
		for (int s = 0; s < DBGK_MAPROW_STREAMS; ++s) {
			if (!total[s]) continue;
			const uint64_t tiles = (total[s] + emitk::kEmitTile - 1) / emitk::kEmitTile;
			const unsigned grid = (unsigned)std::min<uint64_t>(tiles, (uint64_t)r->n_cu * 64);
			const uint32_t two = (s == 0 || (pair && s == 1)) ? 1u : 0u;
			if (!pair && s == 2)
				hipLaunchKernelGGL(rowk::k_maprow_write<true>, dim3(grid), dim3(emitk::kEmitBlock), 0, r->stream, in, (const uint32_t *)r->cls.p,
				                   (const uint8_t *)r->plane.p, (const uint64_t *)r->coff[s].p, (uint32_t)n, total[s], 0u, reinterpret_cast<uint4 *>(r->out[s].p));
			else
				hipLaunchKernelGGL(rowk::k_maprow_write<false>, dim3(grid), dim3(emitk::kEmitBlock), 0, r->stream, in, (const uint32_t *)r->cls.p,
				                   (const uint8_t *)r->plane.p, (const uint64_t *)r->coff[s].p, (uint32_t)n, total[s], two, reinterpret_cast<uint4 *>(r->out[s].p));
			HIPCHK(hipGetLastError());
		}
		HIPCHK(hipEventRecord(r->ev[3], r->stream));
		HIPCHK(hipStreamSynchronize(r->stream));
	}
	dbgk_maprow_info I{};
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, r->ev[0], r->ev[1]));
	I.ms_scan = ms;
	if (any) {
		HIPCHK(hipEventElapsedTime(&ms, r->ev[2], r->ev[3]));
		I.ms_write = ms;
	}
	I.n = n;
	for (int c = 0; c < 5; ++c) I.counters[c] = ctr[rowk::RC_TOTAL + c];
	I.unprintable = ctr[rowk::RC_UNPRINTABLE];
	for (int s = 0; s < DBGK_MAPROW_STREAMS; ++s) I.stream_bytes[s] = r->n_out[s] = total[s];
	r->have = true;
	*out = I;
	return DBGK_OK;
}

// what both calls ask of their arguments; n_sides sides are looked at
static bool maprow_args_ok(const dbgk_maprow *r, const dbgk_maprow_side *sides, uint64_t n, const dbgk_maprow_info *out, bool host_hits)
{
	if (!r || !out || !sides || n >= (1ull << 31)) return false;
	for (int s = 0; s < (r->mode == DBGK_MAPROW_PAIR ? 2 : 1); ++s) {
		const dbgk_maprow_side &H = sides[s];
		if (H.n_text >= (1ull << 31) || (H.n_text && !H.text)) return false;
		if (n && (!H.recs || !H.offsets || (r->mode == DBGK_MAPROW_READS && !H.bases) || (host_hits && !H.hits))) return false; // (PAIR never reads the bases)
	}
	return true;
}

extern "C" int dbgk_maprow_rows_device(dbgk_maprow *r, const dbgk_maprow_side *sides, uint64_t n, dbgk_maprow_info *out)
{
	if (!maprow_args_ok(r, sides, n, out, false)) return DBGK_ERR_ARG;
	const int n_sides = r->mode == DBGK_MAPROW_PAIR ? 2 : 1;
	for (int s = 0; s < n_sides; ++s) {
		const dbgk_maprow_side &H = sides[s];
		if (((uintptr_t)H.text & 15u) || ((uintptr_t)H.bases & 15u) || ((uintptr_t)H.offsets & 7u) || ((uintptr_t)H.recs & 3u)) return DBGK_ERR_ARG;
	}
	r->have = false;
	if (!r->have_contigs) return DBGK_ERR_STATE;
	for (int s = 0; s < n_sides; ++s)
		if (!r->side[s].have_hits || r->side[s].n_hits != n) return DBGK_ERR_STATE;
	HIPCHK(hipSetDevice(r->device));
	return maprow_run(r, sides, n, out);
}

extern "C" int dbgk_maprow_rows(dbgk_maprow *r, const dbgk_maprow_side *sides, uint64_t n, dbgk_maprow_info *out)
{
	if (!maprow_args_ok(r, sides, n, out, true)) return DBGK_ERR_ARG;
	const int n_sides = r->mode == DBGK_MAPROW_PAIR ? 2 : 1;
	for (int s = 0; s < n_sides; ++s) // (the planes are uploaded up to offsets[n])
		for (uint64_t i = 0; i < n; ++i)
			if (sides[s].offsets[i + 1] < sides[s].offsets[i]) return DBGK_ERR_ARG;
	r->have = false;
	if (!r->have_contigs) return DBGK_ERR_STATE;
	HIPCHK(hipSetDevice(r->device));
	HIPCHK(hipStreamSynchronize(r->stream));
	dbgk_maprow_side dev[2] = {};
	for (int s = 0; s < n_sides; ++s) {
		const dbgk_maprow_side &H = sides[s];
		dbgk_maprow::Side &S = r->side[s];
		const uint64_t nb = n && r->mode == DBGK_MAPROW_READS ? H.offsets[n] : 0; // PAIR prints the lengths alone
		if (maprow_hits_reserve(r, s, n) || S.in_text.reserve(H.n_text + 16, 1 << 16) || S.in_b.reserve(nb + 16, 1 << 16) ||
		    S.in_off.reserve((n + 1) * 8, 1 << 14) || S.in_rec.reserve(std::max<uint64_t>(n, 1) * sizeof(dbgk_parse_rec), 1 << 14))
			return DBGK_ERR_NOMEM;
		if (H.n_text) HIPCHK(hipMemcpyAsync(S.in_text, H.text, H.n_text, hipMemcpyHostToDevice, r->stream));
		if (nb) HIPCHK(hipMemcpyAsync(S.in_b, H.bases, nb, hipMemcpyHostToDevice, r->stream));
		if (n) {
			HIPCHK(hipMemcpyAsync(S.in_off, H.offsets, (n + 1) * 8, hipMemcpyHostToDevice, r->stream));
			HIPCHK(hipMemcpyAsync(S.in_rec, H.recs, n * sizeof(dbgk_parse_rec), hipMemcpyHostToDevice, r->stream));
			HIPCHK(hipMemcpyAsync(S.hits, H.hits, 2 * n * sizeof(dbgk_map_hit), hipMemcpyHostToDevice, r->stream));
		}
		S.n_hits = n;
		S.have_hits = true;
		dev[s] = dbgk_maprow_side{(const char *)S.in_text.p, H.n_text, S.in_rec.p, (const char *)S.in_b.p, S.in_off.p, nullptr};
	}
	HIPCHK(hipStreamSynchronize(r->stream)); // the caller's buffers are free on return
	return maprow_run(r, dev, n, out);
}

extern "C" int dbgk_maprow_device(dbgk_maprow *r, int32_t stream, const void **d_text, uint64_t *n_bytes)
{
	if (!r || !d_text || !n_bytes || stream < 0 || stream >= DBGK_MAPROW_STREAMS) return DBGK_ERR_ARG;
	if (!r->have) return DBGK_ERR_STATE;
	*d_text = r->out[stream].p;
	*n_bytes = r->n_out[stream];
	return DBGK_OK;
}

extern "C" int dbgk_maprow_results(dbgk_maprow *r, int32_t stream, void *out, uint64_t capacity)
{
	if (!r || stream < 0 || stream >= DBGK_MAPROW_STREAMS) return DBGK_ERR_ARG;
	if (!r->have) return DBGK_ERR_STATE;
	const uint64_t n = r->n_out[stream];
	if (capacity < n || (n && !out)) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(r->device));
	if (n) HIPCHK(hipMemcpyAsync(out, r->out[stream], n, hipMemcpyDeviceToHost, r->stream));
	HIPCHK(hipStreamSynchronize(r->stream));
	return DBGK_OK;
}
