// SUPER: host side of link_supertig on the GPU (include/dbgk.h, SUPER section; kernels in dbgk_super.h).  A dbgk_super owns a
// dbgk_fill for the records and the table (k_fill_orient, then the LINK sort / reduce / chain, passes and walk with the interleaving
// pass on) and adds its own gap statistics, the slice geometry and the slice read-out.  The sequences go through dbgk_link_emit.

struct dbgk_super {
	dbgk_fill *F = nullptr;
	dbgk_super_params p{};
	std::vector<uint64_t> read_off;                // host copy of the read offsets: the slice geometry needs the lengths only
	bool reads_set = false;
	// gap statistics, ascending by key
	std::vector<superk::PairStat> pairs;
	DevBuf<superk::Counters> d_sctr;
	// dbgk_super_resolve
	bool resolved = false;
	std::vector<uint64_t> scaf_first;
	std::vector<dbgk_link_item> items;
	std::vector<dbgk_super_junction> junctions;
	std::vector<dbgk_super_slice> slices;
	std::vector<int32_t> repeats;
	DevBuf<uint8_t> d_slices;
	uint64_t slice_bytes = 0;
	dbgk_super_summary summary{};
	dbgk_super_timing stats{};
};

static_assert(sizeof(dbgk_super_gapstat) == 32 && sizeof(dbgk_super_junction) == 56 && offsetof(dbgk_super_junction, first_slice) == 40,
              "SUPER statistics layout");
static_assert(sizeof(dbgk_super_slice) == 24 && offsetof(dbgk_super_slice, reversed) == 20, "dbgk_super_slice layout");
static_assert(sizeof(dbgk_super_summary) == 112 && sizeof(dbgk_super_timing) == 88, "SUPER summary layout");
static_assert(sizeof(superk::Acc) == 32 && sizeof(superk::PairStat) == 48 && sizeof(superk::Piece) == 24, "SUPER device descriptors");

extern "C" int dbgk_super_create(const dbgk_super_params *p, int device, dbgk_super **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (!p || device < 0 || p->pair_num_cut < 0 || p->reserved[0] || p->reserved[1] || p->reserved[2]) return DBGK_ERR_ARG;
	dbgk_super *s = new (std::nothrow) dbgk_super;
	if (!s) return DBGK_ERR_NOMEM;
	s->p = *p;
	dbgk_fill_params fp{p->pair_num_cut, {0, 0, 0}};
	int rc = dbgk_fill_create(&fp, device, &s->F);
	if (!rc) rc = s->d_sctr.reserve(sizeof(superk::Counters));
	if (rc) {
		dbgk_super_destroy(s);
		return rc;
	}
	*out = s;
	return DBGK_OK;
}

extern "C" int dbgk_super_destroy(dbgk_super *s)
{
	if (!s) return DBGK_ERR_ARG;
	dbgk_fill *f = s->F;
	if (f) stage_drain(f->L->device, f->L->stream);
	delete s; // (its buffers go before the link's stream does)
	if (f) dbgk_fill_destroy(f);
	return DBGK_OK;
}

extern "C" int dbgk_super_set_contigs(dbgk_super *s, const uint32_t *lengths, uint64_t n_contigs)
{
	if (!s) return DBGK_ERR_ARG;
	return dbgk_fill_set_contigs(s->F, lengths, n_contigs);
}

extern "C" int dbgk_super_set_reads(dbgk_super *s, const char *bases, const uint64_t *offsets, uint64_t n_reads)
{
	if (!s) return DBGK_ERR_ARG;
	if (s->resolved) return DBGK_ERR_STATE;
	const int rc = dbgk_fill_set_reads(s->F, bases, offsets, n_reads);
	if (rc) return rc;
	s->read_off.assign(offsets, offsets + n_reads + 1);
	s->reads_set = true;
	return DBGK_OK;
}

extern "C" int dbgk_super_add_records(dbgk_super *s, const dbgk_fill_record *recs, uint64_t n)
{
	if (!s) return DBGK_ERR_ARG;
	return dbgk_fill_add_records(s->F, recs, n);
}

extern "C" int dbgk_super_add_hits(dbgk_super *s, const dbgk_map_hit *hits, uint64_t n_reads, uint64_t first_read)
{
	if (!s) return DBGK_ERR_ARG;
	return dbgk_fill_add_hits(s->F, hits, n_reads, first_read);
}

extern "C" int dbgk_super_build(dbgk_super *s)
{
	if (!s) return DBGK_ERR_ARG;
	dbgk_fill *f = s->F;
	dbgk_link *l = f->L;
	fillk::Counters fc{};
	int rc = fill_build_table(f, fc);
	if (rc) return rc;
	s->pairs.clear();
	const uint64_t n = f->n_records, pooled = fc.pooled;
	if (!pooled) return DBGK_OK;
	// one stable sort by pair keeps file order inside a pair; records map_reads would not have written sort behind the others
	auto t0 = std::chrono::steady_clock::now();
	if ((rc = dbgk_internal_sort_pairs(f->d_pair_keys, f->d_svals, n, l->stream))) return rc;
	f->stats.ms_sort += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	DevBuf<superk::Acc> d_acc;
	DevBuf<superk::PairStat> d_stat;
	// One accumulator per sorted position, used at the first record of a pair: the reduce finds a pair's accumulator through that
	// position, which every thread learns from the tile scan, so no table from positions to pairs is needed.  One result slot per
	// record too (at most one pair per record).  Both are O(records), 80 bytes per record, freed before this call returns; sizing
	// them by pairs would take an ordered compaction of the head positions first.  Not measured.
	if (d_acc.reserve(pooled * sizeof(superk::Acc)) || d_stat.reserve(pooled * sizeof(superk::PairStat))) return DBGK_ERR_NOMEM;
	auto step = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = hip_fail(e, "dbgk_super_build", __LINE__); };
	superk::Counters sc{};
	step(hipMemsetAsync(d_acc, 0, pooled * sizeof(superk::Acc), l->stream));
	step(hipMemsetAsync(s->d_sctr, 0, sizeof(superk::Counters), l->stream));
	step(hipEventRecord(l->ev[0], l->stream));
	if (!rc) {
		const dim3 grid(link_grid(l, pooled)), block(superk::kSuperThreads);
		hipLaunchKernelGGL(superk::k_super_gapstat<0>, grid, block, 0, l->stream, f->d_pair_keys, f->d_svals, pooled, d_acc);
		hipLaunchKernelGGL(superk::k_super_gapstat<1>, grid, block, 0, l->stream, f->d_pair_keys, f->d_svals, pooled, d_acc);
		hipLaunchKernelGGL(superk::k_super_gappack, grid, block, 0, l->stream, f->d_pair_keys, pooled, d_acc, d_stat, s->d_sctr);
		step(hipGetLastError());
	}
	step(hipEventRecord(l->ev[1], l->stream));
	step(hipMemcpyAsync(&sc, s->d_sctr, sizeof sc, hipMemcpyDeviceToHost, l->stream));
	step(hipStreamSynchronize(l->stream));
	if (!rc) {
		float ms = 0;
		step(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
		s->stats.ms_gapstat = ms;
		s->pairs.resize(sc.pairs);
		step(hipMemcpy(s->pairs.data(), d_stat, sc.pairs * sizeof(superk::PairStat), hipMemcpyDeviceToHost));
	}
	if (rc) return rc;
	// the slots come in no particular order
	std::sort(s->pairs.begin(), s->pairs.end(), [](const superk::PairStat &a, const superk::PairStat &b) { return a.key < b.key; });
	for (const superk::PairStat &q : s->pairs)
		if (q.sum < INT32_MIN || q.sum > INT32_MAX || q.dev > INT32_MAX || q.total > (uint32_t)INT32_MAX) {
			s->pairs.clear();
			return DBGK_ERR_ARG;
		}
	return DBGK_OK;
}

extern "C" int dbgk_super_export(dbgk_super *s, uint64_t *first, dbgk_link_entry *links, uint64_t capacity, uint64_t *n_links,
                                 dbgk_link_counters *counters)
{
	if (!s) return DBGK_ERR_ARG;
	return dbgk_link_export(s->F->L, first, links, capacity, n_links, counters);
}

// mean and mean deviation as decide_gap_size forms them: int divisions, truncating toward zero
static dbgk_super_gapstat super_gapstat(const superk::PairStat &q)
{
	const int32_t total = (int32_t)q.total;
	return dbgk_super_gapstat{(int32_t)(q.key >> 32), (int32_t)(uint32_t)q.key, (int32_t)q.sum / total, q.min, q.max, total, (int32_t)q.dev / total, 0};
}

extern "C" int dbgk_super_gap_stats(dbgk_super *s, dbgk_super_gapstat *out, uint64_t capacity, uint64_t *n_pairs)
{
	if (!s || !n_pairs) return DBGK_ERR_ARG;
	if (!s->F->L->built) return DBGK_ERR_STATE;
	*n_pairs = s->pairs.size();
	if (out) {
		if (capacity < s->pairs.size()) return DBGK_ERR_CAPACITY;
		for (size_t i = 0; i < s->pairs.size(); ++i) out[i] = super_gapstat(s->pairs[i]);
	}
	return DBGK_OK;
}

extern "C" int dbgk_super_resolve(dbgk_super *s, dbgk_super_summary *out)
{
	if (!s || !out) return DBGK_ERR_ARG;
	dbgk_fill *f = s->F;
	dbgk_link *l = f->L;
	if (!l->built) return DBGK_ERR_STATE;
	if (s->resolved) {
		*out = s->summary;
		return DBGK_OK;
	}
	HIPCHK(hipSetDevice(l->device));
	LinkPasses S(l);
	std::vector<std::vector<int>> combs;
	link_passes_and_walk(l, true, S, combs);       // (the snapshots are the link's; it counts as resolved once this call succeeds)
	dbgk_super_summary sum{};
	sum.bad_record = sum.bad_read = -1;
	sum.bad_left = sum.bad_right = -1;
	// the records by pair in file order, as the device sorted them
	const uint64_t pooled = f->n_pooled;
	std::vector<uint64_t> svals(pooled);
	std::vector<int4> rinfo(f->n_records);
	if (pooled) {
		HIPCHK(hipMemcpyAsync(svals.data(), f->d_svals, pooled * 8, hipMemcpyDeviceToHost, l->stream));
		HIPCHK(hipMemcpyAsync(rinfo.data(), f->d_rinfo, f->n_records * sizeof(int4), hipMemcpyDeviceToHost, l->stream));
		HIPCHK(hipStreamSynchronize(l->stream));
	}
	// fill_gaps_inside_scaffold (link_supertig.cpp:364-541) in walk order
	std::vector<std::vector<dbgk_link_item>> scaf;
	std::vector<std::vector<dbgk_super_junction>> scaf_junc;
	std::vector<dbgk_super_slice> slices;
	std::vector<superk::Piece> pieces;
	std::vector<LenIdx> order, by_len;
	uint64_t slice_bytes = 0, lines = 0;
	int32_t gap_id = 0;
	for (const std::vector<int> &comb : combs) {
		std::vector<dbgk_link_item> items;
		std::vector<dbgk_super_junction> junc;
		int scaf_len = 0;
		for (size_t j = 0; j < comb.size(); j += 2) {
			const int id = comb[j];
			const int32_t c = id % 2 == 1 ? id / 2 : (id - 1) / 2;
			const int32_t rev = id % 2 == 1 ? 0 : 1;
			items.push_back(dbgk_link_item{c, rev});
			scaf_len += (int)l->lens[c];
			if (j + 2 >= comb.size()) break;
			const int id2 = comb[j + 2];
			const int32_t c2 = id2 % 2 == 1 ? id2 / 2 : (id2 - 1) / 2;
			const uint32_t dir = rev ? 'R' : 'F', dir2 = id2 % 2 == 1 ? 'F' : 'R';
			const uint64_t key = ((uint64_t)(uint32_t)std::min(c, c2) << 32) | (uint32_t)std::max(c, c2);
			auto it = std::lower_bound(s->pairs.begin(), s->pairs.end(), key, [](const superk::PairStat &q, uint64_t k) { return q.key < k; });
			if (it == s->pairs.end() || it->key != key) return DBGK_ERR_STATE;   // (a link has the records it was made of)
			if (!s->reads_set) return DBGK_ERR_STATE;
			const dbgk_super_gapstat g = super_gapstat(*it);
			dbgk_super_junction J{};
			J.left_contig = c; J.right_contig = c2;
			J.mean = g.mean; J.min = g.min; J.max = g.max; J.total = g.total; J.variance = g.variance;
			J.n_written = g.mean <= 0 ? 1 : g.mean;    // :430-433
			J.gap_id = ++gap_id;
			J.first_slice = slices.size();
			J.n_slices = it->total;
			// one slice per record of the pair, in file order (:443-467); lengths need no bytes
			struct Geo { uint64_t record, src; uint32_t len, rev; };
			std::vector<Geo> geo(it->total);
			by_len.clear();
			const uint64_t n_reads = s->read_off.size() - 1;
			for (uint32_t k = 0; k < it->total; ++k) {
				const uint64_t v = svals[it->first + k], r = v >> 32;
				const int4 ri = rinfo[r];              // read, align1_end, contig1, direct1
				const int64_t a1e = ri.y, a2s = (int64_t)(int32_t)((uint32_t)ri.y + (uint32_t)v + 1u);
				const int64_t gs = a2s > a1e ? a2s - a1e - 1 : 0;
				const int64_t pos = (a1e + a2s) / 2 - 250 - gs / 2;
				const int64_t read_len = (uint64_t)(uint32_t)ri.x < n_reads ? (int64_t)(s->read_off[ri.x + 1] - s->read_off[ri.x]) : -1;
				if (read_len < 0 || pos < 0 || pos > read_len) {   // substr throws
					sum.bad_record = (int64_t)r; sum.bad_read = ri.x; sum.bad_left = c; sum.bad_right = c2;
					*out = sum;
					return DBGK_ERR_ARG;
				}
				const uint32_t len = (uint32_t)std::min<int64_t>(gs + 500, read_len - pos);
				const bool rc = (ri.z == c && (uint32_t)ri.w != dir) || (ri.z == c2 && (uint32_t)ri.w != dir2);   // :459
				geo[k] = Geo{r, s->read_off[ri.x] + (uint64_t)pos, len, rc ? 1u : 0u};
				by_len.push_back(LenIdx{len, k});
			}
			link_sort_by_len(by_len);                  // :469
			const uint32_t median = it->total / 2;
			const uint64_t mlen = by_len[median].len;
			J.median = (int32_t)median;
			// the median's line comes first, then the others in sorted order (:477-495)
			auto put = [&](uint32_t k, uint8_t kept) {
				const Geo &G = geo[by_len[k].idx];
				slices[J.first_slice + k] = dbgk_super_slice{G.record, kept ? slice_bytes : 0, G.len, (uint8_t)G.rev, kept, {0, 0}};
				if (!kept) return;
				lines++;
				J.n_kept++;
				for (uint32_t done = 0; done < G.len;) {
					const uint64_t dst = slice_bytes + done;
					const uint32_t part = std::min<uint32_t>(G.len - done, superk::kPieceBytes - (uint32_t)(dst & 63));
					pieces.push_back(superk::Piece{G.rev ? G.src + (G.len - 1 - done) : G.src + done, dst, part, G.rev});
					done += part;
				}
				slice_bytes += G.len;
			};
			slices.resize(slices.size() + it->total);
			put(median, 2);
			for (uint32_t k = 0; k < it->total; ++k) {
				if (k == median) continue;
				const uint64_t len = by_len[k].len;
				put(k, (double)len > (double)mlen * 0.75 && (double)len < (double)mlen * 1.25 ? 1 : 0);
			}
			items.push_back(dbgk_link_item{-1, J.n_written});
			scaf_len += J.n_written;
			junc.push_back(J);
		}
		// scaf_len is an int in the reference; LenAndSeq.len takes it as uint64_t
		order.push_back(LenIdx{(uint64_t)(int64_t)scaf_len, scaf.size()});
		scaf.push_back(std::move(items));
		scaf_junc.push_back(std::move(junc));
	}
	if (pieces.size() >= (1ull << 32)) return DBGK_ERR_CAPACITY;

	// every written slice in one launch
	s->d_slices.release();
	if (slice_bytes) {
		DevBuf<superk::Piece> d_pieces;
		if (s->d_slices.reserve(slice_bytes + 16) || d_pieces.reserve(pieces.size() * sizeof(superk::Piece))) return DBGK_ERR_NOMEM;
		int rc = DBGK_OK;
		auto step = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = hip_fail(e, "dbgk_super_resolve", __LINE__); };
		step(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(superk::Piece), hipMemcpyHostToDevice, l->stream));
		step(hipEventRecord(l->ev[0], l->stream));
		if (!rc) {
			const uint64_t blocks = (pieces.size() + 3) / 4;   // four waves per block, one piece per wave
			hipLaunchKernelGGL(superk::k_super_slices, dim3((unsigned)std::min<uint64_t>(blocks, (uint64_t)l->n_cu * 16)), dim3(superk::kSuperThreads), 0,
			                   l->stream, d_pieces, (uint64_t)pieces.size(), f->d_reads, s->d_slices);
			step(hipGetLastError());
		}
		step(hipEventRecord(l->ev[1], l->stream));
		step(hipStreamSynchronize(l->stream));
		float ms = 0;
		if (!rc) step(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
		if (rc) return rc;
		s->stats.ms_slices = ms;
	}
	s->slice_bytes = slice_bytes;
	s->slices = std::move(slices);

	link_layout_order(l, S, order, s->repeats);
	s->scaf_first.assign(1, 0);
	s->items.clear();
	s->junctions.clear();
	for (const LenIdx &o : order) {
		s->items.insert(s->items.end(), scaf[o.idx].begin(), scaf[o.idx].end());
		s->junctions.insert(s->junctions.end(), scaf_junc[o.idx].begin(), scaf_junc[o.idx].end());
		s->scaf_first.push_back(s->items.size());
	}
	sum.lowfreq = S.s.lowfreq; sum.interleave = S.s.interleave; sum.repeat_nodes = S.s.repeat_nodes; sum.deleted = S.s.deleted;
	sum.scaffolds = scaf.size(); sum.items = s->items.size(); sum.junctions = s->junctions.size(); sum.slices = s->slices.size();
	sum.lines = lines; sum.slice_bytes = slice_bytes; sum.pairs = s->pairs.size();
	s->summary = sum;
	s->stats.slice_bytes = slice_bytes;
	l->resolved = true;
	s->resolved = true;
	*out = sum;
	return DBGK_OK;
}

extern "C" int dbgk_super_snapshot(dbgk_super *s, int32_t stage, uint8_t *inlink, uint8_t *link, dbgk_link_entry *links)
{
	if (!s || stage < 0 || stage > 1) return DBGK_ERR_ARG;
	if (!s->resolved) return DBGK_ERR_STATE;
	return dbgk_link_snapshot(s->F->L, stage, inlink, link, links);
}

extern "C" int dbgk_super_layout(dbgk_super *s, uint64_t *scaf_first, dbgk_link_item *items, dbgk_super_junction *junctions, int32_t *repeats)
{
	if (!s) return DBGK_ERR_ARG;
	if (!s->resolved) return DBGK_ERR_STATE;
	if (scaf_first) memcpy(scaf_first, s->scaf_first.data(), s->scaf_first.size() * 8);
	if (items && !s->items.empty()) memcpy(items, s->items.data(), s->items.size() * sizeof(dbgk_link_item));
	if (junctions && !s->junctions.empty()) memcpy(junctions, s->junctions.data(), s->junctions.size() * sizeof(dbgk_super_junction));
	if (repeats && !s->repeats.empty()) memcpy(repeats, s->repeats.data(), s->repeats.size() * 4);
	return DBGK_OK;
}

extern "C" int dbgk_super_slices(dbgk_super *s, dbgk_super_slice *out, uint64_t capacity, uint64_t *n_slices)
{
	if (!s || !n_slices) return DBGK_ERR_ARG;
	if (!s->resolved) return DBGK_ERR_STATE;
	*n_slices = s->slices.size();
	if (out) {
		if (capacity < s->slices.size()) return DBGK_ERR_CAPACITY;
		if (!s->slices.empty()) memcpy(out, s->slices.data(), s->slices.size() * sizeof(dbgk_super_slice));
	}
	return DBGK_OK;
}

extern "C" int dbgk_super_slice_bytes(dbgk_super *s, char *out, uint64_t capacity, uint64_t *n_bytes)
{
	if (!s || !n_bytes) return DBGK_ERR_ARG;
	if (!s->resolved) return DBGK_ERR_STATE;
	*n_bytes = s->slice_bytes;
	if (out && s->slice_bytes) {
		if (capacity < s->slice_bytes) return DBGK_ERR_CAPACITY;
		HIPCHK(hipSetDevice(s->F->L->device));
		HIPCHK(hipMemcpy(out, s->d_slices, s->slice_bytes, hipMemcpyDeviceToHost));
	}
	return DBGK_OK;
}

extern "C" int dbgk_super_emit(dbgk_super *s, const char *bases, const uint64_t *offsets, uint64_t n_contigs, const dbgk_link_item *items,
                               uint64_t n_items, char *out, uint64_t capacity, uint64_t *out_len)
{
	if (!s) return DBGK_ERR_ARG;
	return dbgk_link_emit(s->F->L, bases, offsets, n_contigs, items, n_items, out, capacity, out_len);
}

extern "C" int dbgk_super_batch_stats(dbgk_super *s, dbgk_super_timing *out)
{
	if (!s || !out) return DBGK_ERR_ARG;
	const dbgk_fill_timing &ft = s->F->stats;
	const dbgk_link_timing &lt = s->F->L->stats;
	s->stats.records = ft.records; s->stats.pooled = ft.pooled; s->stats.links = ft.links;
	s->stats.ms_orient = ft.ms_orient; s->stats.ms_sort = ft.ms_sort; s->stats.ms_table = ft.ms_table;
	s->stats.ms_emit = lt.ms_emit; s->stats.emit_bytes = lt.emit_bytes;
	*out = s->stats;
	return DBGK_OK;
}
