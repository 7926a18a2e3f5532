// PARSE stage, host side (include/dbgk.h, PARSE section; kernels in dbgk_parse.h): the line table and the scans of one chunk of
// text, and the batch as an EmitStage, so that its read-back, its device view and its hand-over to a graph handle are
// dbgk_host_emit.h's, with its event ordering.  The launches of a chunk follow each other on one stream; the host reads three
// numbers in between (newlines, records, output bytes), each of which sizes what the next launches write.

struct dbgk_parse : StageDev {
	int format = 1;
	bool with_quals = false;
	EmitStage out; // split_src; its counters are parsek::Counter, its scan storage serves every scan of the stage
	DevBuf<uint8_t> text; // dbgk_parse_chunk: the uploaded chunk
	const uint8_t *last_text = nullptr; // the text of the last chunk where it lies (dbgk_parse_text_device)
	uint64_t last_n = 0;
	DevBuf<uint32_t> tile_cnt; // per tile of the text: newlines, and their exclusive scan
	DevBuf<uint64_t> tile_off;
	uint64_t cap_tiles = 0;
	DevBuf<uint32_t> table, flag; // per line (+ 1): the line table, header flags and their exclusive scan
	DevBuf<uint64_t> rank;
	DevBuf<uint8_t> agg, entry; // per kLineChunk lines: the chunk's map, the state it is entered in
	uint64_t cap_lines = 0;
	DevBuf<dbgk_parse_rec> rec;
	DevBuf<parsek::ParseMisc> misc;
	StageEvents<6> ev; // count + scan, lines, states + scan
};

extern "C" int dbgk_parse_create(int32_t format, int32_t with_quals, int device, dbgk_parse **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (device < 0 || (format != 1 && format != 2) || (with_quals && format != 1)) return DBGK_ERR_ARG;
	dbgk_parse *p = new (std::nothrow) dbgk_parse;
	if (!p) return DBGK_ERR_NOMEM;
	p->format = format;
	p->with_quals = with_quals != 0;
	int rc = stage_open(*p, device);
	if (!rc) rc = emit_create(p->out, parsek::PC_COUNT, false);
	p->out.split_src = true;
	if (!rc) rc = p->ev.create();
	if (!rc) rc = p->misc.reserve(sizeof(parsek::ParseMisc));
	if (rc) {
		dbgk_parse_destroy(p);
		return rc;
	}
	*out = p;
	return DBGK_OK;
}

extern "C" int dbgk_parse_destroy(dbgk_parse *p)
{
	if (!p) return DBGK_ERR_ARG;
	stage_drain(p->device, p->stream);
	emit_destroy(p->out);
	delete p;
	return DBGK_OK;
}

// (the stream is idle: every caller has just read a number back)
static int parse_ensure_tiles(dbgk_parse *p, uint64_t n_tiles)
{
	if (n_tiles <= p->cap_tiles && p->tile_cnt) return DBGK_OK;
	p->cap_tiles = 0;
	const uint64_t cap = std::max<uint64_t>(n_tiles, 1 << 10);
	if (p->tile_cnt.reserve((cap + 1) * 4) || p->tile_off.reserve((cap + 1) * 8)) return DBGK_ERR_NOMEM;
	p->cap_tiles = cap;
	return DBGK_OK;
}

// the table's n_lines + 1 entries, and what the map scan keeps per line and per chunk of n_lines + 1 entries
static int parse_ensure_lines(dbgk_parse *p, uint64_t n_lines)
{
	if (n_lines <= p->cap_lines && p->table) return DBGK_OK;
	p->cap_lines = 0;
	const uint64_t cap = std::max<uint64_t>(n_lines, 1 << 16), chunks = (cap + 1 + parsek::kLineChunk - 1) / parsek::kLineChunk;
	if (p->table.reserve((cap + 1) * 4) || p->flag.reserve((cap + 1) * 4) || p->rank.reserve((cap + 1) * 8) || p->agg.reserve(chunks) ||
	    p->entry.reserve(chunks))
		return DBGK_ERR_NOMEM;
	p->cap_lines = cap;
	return DBGK_OK;
}

// one chunk that lies on the device, readable up to n_bytes rounded up to 16 (the stream is ordered behind whatever wrote it)
static int parse_run(dbgk_parse *p, const uint8_t *text, uint64_t n_bytes, bool last, dbgk_parse_info *out)
{
	EmitStage &s = p->out;
	s.have = false;
	p->last_text = text;
	p->last_n = n_bytes;
	const bool fastq = p->format == 1;
	const uint32_t nb = (uint32_t)n_bytes;
	dbgk_parse_info I{};
	uint64_t n_nl = 0, n_lines = 0, n_rec = 0;
	parsek::ParseMisc misc{};
	float ms = 0;
	if (nb) {
		// ---- lines
		const uint32_t n_tiles = (nb + parsek::kTextTile - 1) / parsek::kTextTile;
		const unsigned grid = (unsigned)std::min<uint64_t>(n_tiles, (uint64_t)p->n_cu * 32);
		int rc = parse_ensure_tiles(p, n_tiles);
		if (rc) return rc;
		HIPCHK(hipEventRecord(p->ev[0], p->stream));
		hipLaunchKernelGGL(parsek::k_parse_count, dim3(grid + 1), dim3(parsek::kParseBlock), 0, p->stream, reinterpret_cast<const uint4 *>(text), nb,
		                   n_tiles, p->tile_cnt);
		HIPCHK(hipGetLastError());
		rc = stage_scan(s.tmp, p->stream, p->tile_cnt, p->tile_off, (uint64_t)n_tiles + 1);
		if (rc) return rc;
		HIPCHK(hipEventRecord(p->ev[1], p->stream));
		uint8_t last_byte = 0;
		HIPCHK(hipMemcpyAsync(&n_nl, p->tile_off + n_tiles, 8, hipMemcpyDeviceToHost, p->stream));
		HIPCHK(hipMemcpyAsync(&last_byte, text + nb - 1, 1, hipMemcpyDeviceToHost, p->stream));
		HIPCHK(hipStreamSynchronize(p->stream)); // the number of newlines sizes the line table
		// with last == 0 a line is what ends with a newline; else the bytes behind the last newline are a line too
		n_lines = n_nl + ((last && last_byte != '\n') ? 1 : 0);
		rc = parse_ensure_lines(p, n_nl + 1);
		if (rc) return rc;
		HIPCHK(hipEventRecord(p->ev[2], p->stream));
		hipLaunchKernelGGL(parsek::k_parse_lines, dim3(grid), dim3(parsek::kParseBlock), 0, p->stream, text, nb, n_tiles, (const uint64_t *)p->tile_off,
		                   (uint32_t)(fastq ? '@' : '>'), p->table);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(p->ev[3], p->stream));
		// ---- states
		HIPCHK(hipMemsetAsync(p->misc, 0, sizeof misc, p->stream));
		const uint32_t chunks = (uint32_t)((n_lines + 1 + parsek::kLineChunk - 1) / parsek::kLineChunk);
		HIPCHK(hipEventRecord(p->ev[4], p->stream));
		hipLaunchKernelGGL(parsek::k_parse_map_reduce, dim3(chunks), dim3(parsek::kParseBlock), 0, p->stream, (const uint32_t *)p->table,
		                   (uint32_t)n_lines, (uint32_t)fastq, p->agg);
		hipLaunchKernelGGL(parsek::k_parse_map_spine, dim3(1), dim3(parsek::kParseBlock), 0, p->stream, (const uint8_t *)p->agg, chunks, p->entry, p->misc);
		hipLaunchKernelGGL(parsek::k_parse_states, dim3(chunks), dim3(parsek::kParseBlock), 0, p->stream, (const uint32_t *)p->table, (uint32_t)n_lines,
		                   (uint32_t)fastq, (const uint8_t *)p->entry, p->flag, p->misc);
		HIPCHK(hipGetLastError());
		rc = stage_scan(s.tmp, p->stream, p->flag, p->rank, n_lines + 1);
		if (rc) return rc;
		HIPCHK(hipEventRecord(p->ev[5], p->stream));
		HIPCHK(hipMemcpyAsync(&n_rec, p->rank + n_lines, 8, hipMemcpyDeviceToHost, p->stream));
		HIPCHK(hipMemcpyAsync(&misc, p->misc, sizeof misc, hipMemcpyDeviceToHost, p->stream));
		HIPCHK(hipStreamSynchronize(p->stream)); // the number of records sizes the batch
		HIPCHK(hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
		I.ms_lines = ms;
		HIPCHK(hipEventElapsedTime(&ms, p->ev[2], p->ev[3]));
		I.ms_lines += ms;
		HIPCHK(hipEventElapsedTime(&ms, p->ev[4], p->ev[5]));
		I.ms_states = ms;
	}
	// With last == 0 the text may end inside a record (a state other than 0 behind its last whole line): that record, the last
	// one, is not delivered, and the caller presents the bytes from its header on again.
	I.consumed = n_bytes;
	I.n_lines = n_lines;
	if (!last) {
		const bool cut = misc.final_state != 0;
		if (cut) {
			n_rec -= 1;
			I.n_lines = (misc.last_head >> 32) - 1;
			I.consumed = misc.last_head & 0xFFFFFFFFull;
		} else if (n_nl) {
			uint32_t e = 0; // the entry behind the last newline: where the unfinished line starts
			HIPCHK(hipMemcpyAsync(&e, p->table + n_nl, 4, hipMemcpyDeviceToHost, p->stream));
			HIPCHK(hipStreamSynchronize(p->stream));
			I.consumed = e & ~parsek::kMarkerBit;
		} else {
			I.consumed = 0;
		}
	}
	if (p->rec.reserve(n_rec * sizeof(dbgk_parse_rec), (1 << 14) * sizeof(dbgk_parse_rec))) return DBGK_ERR_NOMEM;
	unsigned long long ctr[parsek::PC_COUNT] = {0};
	const uint32_t n_lines32 = (uint32_t)n_lines, n_nl32 = (uint32_t)n_nl, n32 = (uint32_t)n_rec;
	const uint64_t line_blocks = (n_lines + parsek::kParseBlock) / parsek::kParseBlock;
	// the record kernel runs over the LINES, so its grid is sized here by them, not by emit_run's count of reads
	auto launch_len = [&](unsigned, uint32_t *len, uint64_t *src, unsigned long long *d_ctr) {
		hipLaunchKernelGGL(parsek::k_parse_records, dim3((unsigned)std::min<uint64_t>(line_blocks, (uint64_t)p->n_cu * 16)), dim3(parsek::kParseBlock), 0,
		                   p->stream, (const uint32_t *)p->table, (const uint32_t *)p->flag, (const uint64_t *)p->rank, n_lines32, n_nl32, nb, n32,
		                   (uint32_t)fastq, (uint32_t)p->with_quals, parsek::ParseOut{p->rec.p, len, src, s.qsrc.p}, d_ctr);
	};
	int rc = emit_run(s, p->stream, p->n_cu, n_rec, text, p->with_quals ? text : nullptr, false, 0u, launch_len, ctr, &I.ms_scan, &I.ms_gather);
	if (rc) return rc;
	I.n_records = n_rec;
	I.ignored_lines = misc.ignored;
	I.n_bases = s.total;
	I.max_len = ctr[parsek::PC_MAX_LEN];
	I.mismatched = ctr[parsek::PC_MISMATCHED];
	*out = I;
	return DBGK_OK;
}

extern "C" int dbgk_parse_chunk_device(dbgk_parse *p, const char *d_text, uint64_t n_bytes, int32_t last, dbgk_parse_info *out)
{
	if (!p || !out || n_bytes >= (1ull << 31) || (n_bytes && !d_text) || ((uintptr_t)d_text & 15u)) return DBGK_ERR_ARG;
	const uint8_t *u = (const uint8_t *)d_text;
	for (const uint8_t *own : {p->out.bases.p, p->out.quals.p}) // the batch the call is about to write
		if (u && own && u + n_bytes > own && u < own + p->out.cap_bytes) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(p->device));
	return parse_run(p, u, n_bytes, last != 0, out);
}

extern "C" int dbgk_parse_chunk(dbgk_parse *p, const char *text, uint64_t n_bytes, int32_t last, dbgk_parse_info *out)
{
	if (!p || !out || n_bytes >= (1ull << 31) || (n_bytes && !text)) return DBGK_ERR_ARG;
	p->out.have = false;
	HIPCHK(hipSetDevice(p->device));
	if (n_bytes + 16 > p->text.cap) {
		HIPCHK(hipStreamSynchronize(p->stream));
		if (p->text.reserve(n_bytes + 16, 1 << 20)) return DBGK_ERR_NOMEM;
	}
	if (n_bytes) HIPCHK(hipMemcpyAsync(p->text, text, n_bytes, hipMemcpyHostToDevice, p->stream));
	HIPCHK(hipStreamSynchronize(p->stream)); // the caller's buffer is free on return
	return parse_run(p, p->text, n_bytes, last != 0, out);
}

extern "C" int dbgk_parse_results(dbgk_parse *p, char *bases, char *quals, uint64_t *offsets, dbgk_parse_rec *recs)
{
	if (!p) return DBGK_ERR_ARG;
	EmitStage &s = p->out;
	if (!s.have) return DBGK_ERR_STATE;
	if (quals && !s.has_qual) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(p->device));
	if (recs && s.n) HIPCHK(hipMemcpyAsync(recs, p->rec, s.n * sizeof(dbgk_parse_rec), hipMemcpyDeviceToHost, p->stream));
	return emit_results(s, p->stream, bases, quals, offsets);
}

extern "C" int dbgk_parse_device(dbgk_parse *p, const char **d_bases, const char **d_quals, const uint64_t **d_offsets, uint64_t *n_reads,
                                 uint64_t *n_bases)
{
	if (!p || !d_bases || !d_quals || !d_offsets || !n_reads || !n_bases) return DBGK_ERR_ARG;
	if (!p->out.have) return DBGK_ERR_STATE;
	emit_device(p->out, d_bases, d_quals, d_offsets, n_reads, n_bases);
	return DBGK_OK;
}

extern "C" int dbgk_push_parsed(dbgk_handle *h, dbgk_parse *p)
{
	if (!h || !p) return DBGK_ERR_ARG;
	if (h->device != p->device) return DBGK_ERR_ARG;
	return emit_push(h, p->out);
}
