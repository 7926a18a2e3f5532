// FILL: host side of link_contig on the GPU (include/dbgk.h, FILL section; kernels in dbgk_fill.h).  A dbgk_fill owns a dbgk_link
// for the table (its entries are written by k_fill_orient; sort, reduce, chain, the host passes and the walk are the LINK ones) and
// adds the gap statistics, the consensus and its own read-out.

struct dbgk_fill {
	dbgk_link *L = nullptr;
	dbgk_fill_params p{};
	// per record, in record order
	DevBuf<uint64_t> d_pair_keys, d_skeys, d_svals;
	DevBuf<int4> d_rinfo;
	uint64_t n_records = 0, cap_records = 0;
	DevBuf<fillk::Counters> d_fctr;
	// reads
	DevBuf<uint8_t> d_reads;
	DevBuf<uint64_t> d_read_off;
	uint64_t n_reads = 0;
	bool reads_set = false;
	// gap statistics, ascending by key
	std::vector<fillk::PairStat> pairs;
	uint64_t n_pooled = 0;
	// dbgk_fill_resolve
	bool resolved = false;
	std::vector<uint64_t> scaf_first;
	std::vector<dbgk_fill_item> items;
	std::vector<dbgk_fill_gap> gaps;
	std::vector<int32_t> repeats;
	DevBuf<uint8_t> d_cons;
	uint64_t cons_bytes = 0;
	dbgk_fill_summary summary{};
	dbgk_fill_timing stats{};
};

static_assert(sizeof(dbgk_fill_record) == 32 && sizeof(fillk::Rec) == 32 && offsetof(dbgk_fill_record, direct1) == 24, "dbgk_fill_record layout");
static_assert(sizeof(dbgk_fill_item) == 24 && offsetof(dbgk_fill_item, cons_off) == 16, "dbgk_fill_item layout");
static_assert(sizeof(dbgk_fill_gapstat) == 24 && sizeof(dbgk_fill_gap) == 24 && sizeof(fillk::PairStat) == 32, "gap statistics layout");
static_assert(sizeof(fillk::GapDesc) == 40 && sizeof(fillk::EmitItem) == 16, "device descriptors");

extern "C" int dbgk_fill_create(const dbgk_fill_params *p, int device, dbgk_fill **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (!p || device < 0 || p->pair_num_cut < 0 || p->reserved[0] || p->reserved[1] || p->reserved[2]) return DBGK_ERR_ARG;
	dbgk_fill *f = new (std::nothrow) dbgk_fill;
	if (!f) return DBGK_ERR_NOMEM;
	f->p = *p;
	dbgk_link_params lp{0, p->pair_num_cut, 1};    // (the orientation and gap of a record are FILL's own: no -m, no -i)
	int rc = dbgk_link_create(&lp, device, &f->L);
	if (!rc) rc = f->d_fctr.reserve(sizeof(fillk::Counters));
	if (!rc && hipMemsetAsync(f->d_fctr, 0, sizeof(fillk::Counters), f->L->stream) != hipSuccess) rc = DBGK_ERR_HIP;
	if (rc) {
		dbgk_fill_destroy(f);
		return rc;
	}
	*out = f;
	return DBGK_OK;
}

extern "C" int dbgk_fill_destroy(dbgk_fill *f)
{
	if (!f) return DBGK_ERR_ARG;
	dbgk_link *l = f->L;
	if (l) stage_drain(l->device, l->stream);
	delete f; // (its buffers go before the link's stream does)
	if (l) dbgk_link_destroy(l);
	return DBGK_OK;
}

extern "C" int dbgk_fill_set_contigs(dbgk_fill *f, const uint32_t *lengths, uint64_t n_contigs)
{
	if (!f) return DBGK_ERR_ARG;
	return dbgk_link_set_contigs(f->L, lengths, n_contigs);
}

extern "C" int dbgk_fill_set_reads(dbgk_fill *f, const char *bases, const uint64_t *offsets, uint64_t n_reads)
{
	if (!f || n_reads >= (1ull << 31) || !link_check_offsets(bases, offsets, n_reads)) return DBGK_ERR_ARG;
	if (f->resolved) return DBGK_ERR_STATE;
	dbgk_link *l = f->L;
	HIPCHK(hipSetDevice(l->device));
	f->reads_set = false;
	f->d_reads.release(); f->d_read_off.release();
	const uint64_t nb = offsets[n_reads];
	if (f->d_reads.reserve(nb + 16) || f->d_read_off.reserve((n_reads + 1) * 8)) return DBGK_ERR_NOMEM;
	if (nb) HIPCHK(hipMemcpyAsync(f->d_reads, bases, nb, hipMemcpyHostToDevice, l->stream));
	HIPCHK(hipMemcpyAsync(f->d_read_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, l->stream));
	HIPCHK(hipStreamSynchronize(l->stream));
	f->n_reads = n_reads;
	f->reads_set = true;
	return DBGK_OK;
}

// room for n_new more records in the per-record arrays
static int fill_reserve(dbgk_fill *f, uint64_t n_new)
{
	if (f->n_records + n_new <= f->cap_records) return DBGK_OK;
	dbgk_link *l = f->L;
	const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(f->n_records + n_new, 2 * f->cap_records), 1 << 15);
	DevBuf<uint64_t> pk, sk, sv;
	DevBuf<int4> ri;
	if (pk.reserve(cap * 8) || sk.reserve(cap * 8) || sv.reserve(cap * 8) || ri.reserve(cap * 16)) return DBGK_ERR_NOMEM;
	if (f->n_records) {
		HIPCHK(hipMemcpyAsync(pk, f->d_pair_keys, f->n_records * 8, hipMemcpyDeviceToDevice, l->stream));
		HIPCHK(hipMemcpyAsync(sk, f->d_skeys, f->n_records * 8, hipMemcpyDeviceToDevice, l->stream));
		HIPCHK(hipMemcpyAsync(sv, f->d_svals, f->n_records * 8, hipMemcpyDeviceToDevice, l->stream));
		HIPCHK(hipMemcpyAsync(ri, f->d_rinfo, f->n_records * 16, hipMemcpyDeviceToDevice, l->stream));
	}
	HIPCHK(hipStreamSynchronize(l->stream));
	f->d_pair_keys.take(pk);
	f->d_skeys.take(sk);
	f->d_svals.take(sv);
	f->d_rinfo.take(ri);
	f->cap_records = cap;
	return DBGK_OK;
}

static int fill_add(dbgk_fill *f, const void *src, uint64_t n, bool from_hits, uint64_t first_read)
{
	dbgk_link *l = f->L;
	if (l->n_entries + 2 * n >= (1ull << 32)) return DBGK_ERR_CAPACITY;   // an entry's index is kept in 32 bits
	if (!l->contigs_set || l->built) return DBGK_ERR_STATE;
	if (!n) return DBGK_OK;
	HIPCHK(hipSetDevice(l->device));
	const uint64_t bytes = n * (from_hits ? 64 : 32);
	int rc = link_reserve(l, 2 * n, bytes);
	if (!rc) rc = fill_reserve(f, n);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(l->d_in, src, bytes, hipMemcpyHostToDevice, l->stream));
	HIPCHK(hipEventRecord(l->ev[0], l->stream));
	const uint32_t nc = (uint32_t)l->lens.size();
	if (from_hits)
		hipLaunchKernelGGL(fillk::k_fill_orient<true>, dim3(link_grid(l, n)), dim3(fillk::kFillThreads), 0, l->stream, (const fillk::Rec *)nullptr,
		                   reinterpret_cast<const linkk::Hit *>(l->d_in.p), n, nc, (uint32_t)first_read, f->n_records, l->d_keys, l->d_vals, f->d_pair_keys,
		                   f->d_skeys, f->d_svals, f->d_rinfo, l->d_ctr, f->d_fctr);
	else
		hipLaunchKernelGGL(fillk::k_fill_orient<false>, dim3(link_grid(l, n)), dim3(fillk::kFillThreads), 0, l->stream,
		                   reinterpret_cast<const fillk::Rec *>(l->d_in.p), (const linkk::Hit *)nullptr, n, nc, 0u, f->n_records, l->d_keys, l->d_vals,
		                   f->d_pair_keys, f->d_skeys, f->d_svals, f->d_rinfo, l->d_ctr, f->d_fctr);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(l->ev[1], l->stream));
	HIPCHK(hipStreamSynchronize(l->stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
	f->stats.ms_orient += ms;
	f->stats.records += n;
	f->n_records += n;
	l->n_entries += 2 * n;
	return DBGK_OK;
}

extern "C" int dbgk_fill_add_records(dbgk_fill *f, const dbgk_fill_record *recs, uint64_t n)
{
	if (!f || (n && !recs) || n >= (1ull << 31)) return DBGK_ERR_ARG;
	const uint64_t nc = f->L->lens.size();
	for (uint64_t i = 0; i < n; ++i)
		if ((uint64_t)(uint32_t)recs[i].contig1 >= nc || (uint64_t)(uint32_t)recs[i].contig2 >= nc || recs[i].contig1 == recs[i].contig2 ||
		    recs[i].read < 0)
			return DBGK_ERR_ARG;
	return fill_add(f, recs, n, false, 0);
}

extern "C" int dbgk_fill_add_hits(dbgk_fill *f, const dbgk_map_hit *hits, uint64_t n_reads, uint64_t first_read)
{
	if (!f || (n_reads && !hits) || n_reads >= (1ull << 31) || first_read + n_reads >= (1ull << 31)) return DBGK_ERR_ARG;
	return fill_add(f, hits, n_reads, true, first_read);
}

// the link table of dbgk_fill_build and dbgk_super_build, and the number of records that take part in the gap statistics
static int fill_build_table(dbgk_fill *f, fillk::Counters &fc)
{
	dbgk_link *l = f->L;
	if (!l->contigs_set || l->built) return DBGK_ERR_STATE;
	int rc = dbgk_link_build(l);
	if (rc) return rc;
	f->stats.ms_sort = l->stats.ms_sort;
	f->stats.ms_table = l->stats.ms_reduce + l->stats.ms_chain;
	f->stats.links = l->stats.links;
	HIPCHK(hipMemcpyAsync(&fc, f->d_fctr, sizeof fc, hipMemcpyDeviceToHost, l->stream));
	HIPCHK(hipStreamSynchronize(l->stream));
	f->n_pooled = fc.pooled;
	f->stats.pooled = fc.pooled;
	return DBGK_OK;
}

extern "C" int dbgk_fill_build(dbgk_fill *f)
{
	if (!f) return DBGK_ERR_ARG;
	dbgk_link *l = f->L;
	// the gap statistics: stable sort by gap, then by pair (records map_reads would not have written sort behind the others)
	fillk::Counters fc{};
	int rc = fill_build_table(f, fc);
	if (rc) return rc;
	f->pairs.clear();
	const uint64_t n = f->n_records;
	if (!fc.pooled) return DBGK_OK;
	auto t0 = std::chrono::steady_clock::now();
	if ((rc = dbgk_internal_sort_pairs(f->d_skeys, f->d_svals, n, l->stream))) return rc;
	f->stats.ms_sort += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	float ms = 0;
	HIPCHK(hipEventRecord(l->ev[0], l->stream));
	hipLaunchKernelGGL(fillk::k_fill_gather, dim3(link_grid(l, n)), dim3(fillk::kFillThreads), 0, l->stream, f->d_svals, f->d_pair_keys, n, f->d_skeys);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(l->ev[1], l->stream));
	HIPCHK(hipStreamSynchronize(l->stream));
	HIPCHK(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
	f->stats.ms_gapstat += ms;
	t0 = std::chrono::steady_clock::now();
	if ((rc = dbgk_internal_sort_pairs(f->d_skeys, f->d_svals, n, l->stream))) return rc;
	f->stats.ms_sort += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	DevBuf<fillk::PairStat> d_stat;
	if (d_stat.reserve(fc.pooled * sizeof(fillk::PairStat))) return DBGK_ERR_NOMEM;   // at most one pair per record
	auto step = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = hip_fail(e, "dbgk_fill_build", __LINE__); };
	step(hipEventRecord(l->ev[0], l->stream));
	hipLaunchKernelGGL(fillk::k_fill_gapstat, dim3(link_grid(l, fc.pooled)), dim3(fillk::kFillThreads), 0, l->stream, f->d_skeys, f->d_svals, fc.pooled,
	                   d_stat, f->d_fctr);
	step(hipGetLastError());
	step(hipEventRecord(l->ev[1], l->stream));
	step(hipMemcpyAsync(&fc, f->d_fctr, sizeof fc, hipMemcpyDeviceToHost, l->stream));
	step(hipStreamSynchronize(l->stream));
	if (!rc) {
		step(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
		f->stats.ms_gapstat += ms;
		f->pairs.resize(fc.pairs);
		step(hipMemcpy(f->pairs.data(), d_stat, fc.pairs * sizeof(fillk::PairStat), hipMemcpyDeviceToHost));
	}
	if (rc) return rc;
	// the slots come in no particular order
	std::sort(f->pairs.begin(), f->pairs.end(), [](const fillk::PairStat &a, const fillk::PairStat &b) { return a.key < b.key; });
	return DBGK_OK;
}

extern "C" int dbgk_fill_export(dbgk_fill *f, uint64_t *first, dbgk_link_entry *links, uint64_t capacity, uint64_t *n_links,
                                dbgk_link_counters *counters)
{
	if (!f) return DBGK_ERR_ARG;
	return dbgk_link_export(f->L, first, links, capacity, n_links, counters);
}

extern "C" int dbgk_fill_gap_stats(dbgk_fill *f, dbgk_fill_gapstat *out, uint64_t capacity, uint64_t *n_pairs)
{
	if (!f || !n_pairs) return DBGK_ERR_ARG;
	if (!f->L->built) return DBGK_ERR_STATE;
	*n_pairs = f->pairs.size();
	if (out) {
		if (capacity < f->pairs.size()) return DBGK_ERR_CAPACITY;
		for (size_t i = 0; i < f->pairs.size(); ++i) {
			const fillk::PairStat &s = f->pairs[i];
			out[i] = dbgk_fill_gapstat{(int32_t)(s.key >> 32), (int32_t)(uint32_t)s.key, s.mode, s.mode_freq, s.total_freq, s.variance};
		}
	}
	return DBGK_OK;
}

// the counted path of a gap whose slices hold bytes other than A C G T N: map<char,int> per column as the reference has it
// (link_contig.cpp:488-509).  The slices come from the device copy of the reads.
static int fill_host_consensus(dbgk_fill *f, const fillk::GapDesc &G, std::vector<uint8_t> &cons, std::vector<uint32_t> &freq)
{
	dbgk_link *l = f->L;
	std::vector<uint64_t> sv(G.n_span);
	HIPCHK(hipMemcpy(sv.data(), f->d_svals + G.span_start, G.n_span * 8ull, hipMemcpyDeviceToHost));
	const uint32_t gap = (uint32_t)G.gap;
	std::vector<uint32_t> count((size_t)gap * 256, 0);
	std::vector<uint8_t> slice(gap);
	for (uint32_t m = 0; m < G.n_span; ++m) {
		int4 r;
		uint64_t off = 0;
		HIPCHK(hipMemcpy(&r, f->d_rinfo + (sv[m] >> 32), sizeof r, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(&off, f->d_read_off + r.x, 8, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(slice.data(), f->d_reads + off + (uint64_t)r.y, gap, hipMemcpyDeviceToHost));
		const bool rc = (r.z == G.left_contig && (uint32_t)r.w != G.left_direct) || (r.z == G.right_contig && (uint32_t)r.w != G.right_direct);
		for (uint32_t k = 0; k < gap; ++k) {
			uint8_t c = slice[k];
			uint32_t col = k;
			if (rc) { // rev_com_seq, seqKmer.cpp:83-91
				col = gap - 1 - k;
				const uint8_t u = c & 0xdf;
				c = (c == 'N' || c == 'n') ? c : u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N';
			}
			count[(size_t)col * 256 + c]++;
		}
	}
	(void)l;
	cons.assign(gap, 0);
	freq.assign(gap, 0);
	for (uint32_t k = 0; k < gap; ++k) {
		// map<char,int> iterates in the order of signed char: 128..255 first
		for (int v = -128; v < 128; ++v) {
			const uint32_t n = count[(size_t)k * 256 + (uint8_t)v];
			if (n > freq[k]) { freq[k] = n; cons[k] = (uint8_t)v; }
		}
	}
	return DBGK_OK;
}

extern "C" int dbgk_fill_resolve(dbgk_fill *f, dbgk_fill_summary *out)
{
	if (!f || !out) return DBGK_ERR_ARG;
	dbgk_link *l = f->L;
	if (!l->built) return DBGK_ERR_STATE;
	if (f->resolved) {
		*out = f->summary;
		return DBGK_OK;
	}
	HIPCHK(hipSetDevice(l->device));
	LinkPasses S(l);
	std::vector<std::vector<int>> combs;
	link_passes_and_walk(l, false, S, combs);
	l->resolved = true;                            // (the snapshots are the link's)
	// the layout in walk order (fill_gaps_inside_scaffold, link_contig.cpp:372-551)
	std::vector<std::vector<dbgk_fill_item>> scaf;
	std::vector<dbgk_fill_gap> gaps;
	std::vector<fillk::GapDesc> desc;              // the filled gaps
	std::vector<uint32_t> desc_gap;                // ... and their index in gaps
	std::vector<LenIdx> order;
	uint64_t cons_bytes = 0, span_bytes = 0;
	for (const std::vector<int> &comb : combs) {
		std::vector<dbgk_fill_item> items;
		int scaf_len = 0;
		for (size_t j = 0; j < comb.size(); j += 2) {
			const int id = comb[j];
			const int32_t c = id % 2 == 1 ? id / 2 : (id - 1) / 2;
			const int32_t rev = id % 2 == 1 ? 0 : 1;
			const int ctg_len = (int)l->lens[c];
			if (j + 2 >= comb.size()) {
				items.push_back(dbgk_fill_item{c, rev, (uint32_t)ctg_len, -1, 0});
				scaf_len += ctg_len;
				break;
			}
			const int id2 = comb[j + 2];
			const int32_t c2 = id2 % 2 == 1 ? id2 / 2 : (id2 - 1) / 2;
			const uint64_t key = ((uint64_t)(uint32_t)std::min(c, c2) << 32) | (uint32_t)std::max(c, c2);
			auto it = std::lower_bound(f->pairs.begin(), f->pairs.end(), key, [](const fillk::PairStat &s, uint64_t k) { return s.key < k; });
			if (it == f->pairs.end() || it->key != key) return DBGK_ERR_STATE;   // (a link has the records it was made of)
			dbgk_fill_gap g{it->mode, it->mode_freq, it->total_freq, it->variance, 0.0f, 0};
			if (it->mode <= 0) {
				// ctg_seq.substr(0, ctg_len + gap_size): a negative length is a huge size_t and keeps the whole contig (:441)
				const int keep = ctg_len + it->mode < 0 ? ctg_len : ctg_len + it->mode;
				items.push_back(dbgk_fill_item{c, rev, (uint32_t)keep, -1, 0});
				items.push_back(dbgk_fill_item{-1, 0, 0, (int32_t)gaps.size(), 0});
				scaf_len += keep;
			} else {
				items.push_back(dbgk_fill_item{c, rev, (uint32_t)ctg_len, -1, 0});
				items.push_back(dbgk_fill_item{-1, 0, (uint32_t)it->mode, (int32_t)gaps.size(), cons_bytes});
				scaf_len += ctg_len + it->mode;
				fillk::GapDesc d;
				d.span_start = it->mode_start;
				d.cons_off = cons_bytes;
				d.n_span = (uint32_t)it->mode_freq;
				d.gap = it->mode;
				d.left_contig = c;
				d.right_contig = c2;
				d.left_direct = rev ? 'R' : 'F';
				d.right_direct = id2 % 2 == 1 ? 'F' : 'R';
				desc.push_back(d);
				desc_gap.push_back((uint32_t)gaps.size());
				cons_bytes += (uint64_t)it->mode;
				span_bytes += (uint64_t)it->mode * (uint64_t)it->mode_freq;
			}
			gaps.push_back(g);
		}
		// scaf_len is an int in the reference; LenAndSeq.len takes it as uint64_t
		order.push_back(LenIdx{(uint64_t)(int64_t)scaf_len, scaf.size()});
		scaf.push_back(std::move(items));
	}
	if (!desc.empty() && !f->reads_set) return DBGK_ERR_STATE;
	if (desc.size() >= (1ull << 31)) return DBGK_ERR_CAPACITY;

	// the consensus of every filled gap in one launch: a work unit is 64 columns of one gap
	if (!desc.empty()) {
		std::vector<uint2> work;
		for (size_t g = 0; g < desc.size(); ++g)
			for (uint32_t b = 0; b < ((uint32_t)desc[g].gap + 63) / 64; ++b) work.push_back(make_uint2((uint32_t)g, b));
		DevBuf<fillk::GapDesc> d_desc;
		DevBuf<uint2> d_work;
		DevBuf<uint32_t> d_freq;
		DevBuf<int> d_status;
		f->d_cons.release();
		if (f->d_cons.reserve(cons_bytes + 16) || d_desc.reserve(desc.size() * sizeof(fillk::GapDesc)) || d_work.reserve(work.size() * sizeof(uint2)) ||
		    d_freq.reserve(cons_bytes * 4) || d_status.reserve(desc.size() * 4))
			return DBGK_ERR_NOMEM;
		int rc = DBGK_OK;
		auto step = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = hip_fail(e, "dbgk_fill_resolve", __LINE__); };
		std::vector<int> status(desc.size(), 0);
		std::vector<uint32_t> freq(cons_bytes);
		step(hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(fillk::GapDesc), hipMemcpyHostToDevice, l->stream));
		step(hipMemcpyAsync(d_work, work.data(), work.size() * sizeof(uint2), hipMemcpyHostToDevice, l->stream));
		step(hipMemsetAsync(d_status, 0, desc.size() * 4, l->stream));
		step(hipEventRecord(l->ev[0], l->stream));
		if (!rc) {
			const uint64_t blocks = (work.size() + 3) / 4;   // four waves per block, one unit per wave
			hipLaunchKernelGGL(fillk::k_fill_consensus, dim3((unsigned)std::min<uint64_t>(blocks, (uint64_t)l->n_cu * 16)), dim3(fillk::kFillThreads), 0,
			                   l->stream, d_work, (uint64_t)work.size(), d_desc, f->d_svals, f->d_rinfo, f->d_reads, f->d_read_off, (uint32_t)f->n_reads,
			                   f->d_cons, d_freq, d_status);
			step(hipGetLastError());
		}
		step(hipEventRecord(l->ev[1], l->stream));
		step(hipMemcpyAsync(status.data(), d_status, desc.size() * 4, hipMemcpyDeviceToHost, l->stream));
		step(hipMemcpyAsync(freq.data(), d_freq, cons_bytes * 4, hipMemcpyDeviceToHost, l->stream));
		step(hipStreamSynchronize(l->stream));
		float ms = 0;
		if (!rc) step(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
		if (rc) return rc;
		f->stats.ms_consensus = ms;
		for (size_t g = 0; g < desc.size(); ++g)
			if (status[g] == fillk::kStatusBadSlice) return DBGK_ERR_ARG;
		for (size_t g = 0; g < desc.size(); ++g) {
			const fillk::GapDesc &G = desc[g];
			if (status[g] == fillk::kStatusHostPath) {
				std::vector<uint8_t> hc;
				std::vector<uint32_t> hf;
				if ((rc = fill_host_consensus(f, G, hc, hf))) return rc;
				std::copy(hf.begin(), hf.end(), freq.begin() + G.cons_off);
				HIPCHK(hipMemcpy(f->d_cons + G.cons_off, hc.data(), hc.size(), hipMemcpyHostToDevice));
				gaps[desc_gap[g]].host_path = 1;
			}
			// ConsensusSupportRate += (float)consensus_freq / total_freq, column 0 first; then /= gap_size (:507-510)
			float rate = 0.0f;
			for (int k = 0; k < G.gap; ++k) rate += (float)(int)freq[G.cons_off + k] / (int)G.n_span;
			rate /= G.gap;
			gaps[desc_gap[g]].identity = rate;
		}
	}
	f->cons_bytes = cons_bytes;

	link_layout_order(l, S, order, f->repeats);
	f->scaf_first.assign(1, 0);
	f->items.clear();
	f->gaps.clear();
	for (const LenIdx &o : order) {
		for (dbgk_fill_item it : scaf[o.idx]) {
			if (it.contig < 0) {                   // the junctions are renumbered in output order
				f->gaps.push_back(gaps[it.gap]);
				it.gap = (int32_t)f->gaps.size() - 1;
			}
			f->items.push_back(it);
		}
		f->scaf_first.push_back(f->items.size());
	}
	f->summary = dbgk_fill_summary{S.s.lowfreq, S.s.repeat_nodes, S.s.deleted, scaf.size(), f->items.size(), f->gaps.size(), desc.size(), cons_bytes,
	                               f->pairs.size()};
	f->stats.cons_bytes = cons_bytes;
	f->stats.span_bytes = span_bytes;
	f->resolved = true;
	*out = f->summary;
	return DBGK_OK;
}

extern "C" int dbgk_fill_snapshot(dbgk_fill *f, int32_t stage, uint8_t *inlink, uint8_t *link, dbgk_link_entry *links)
{
	if (!f || stage < 0 || stage > 1) return DBGK_ERR_ARG;
	if (!f->resolved) return DBGK_ERR_STATE;
	return dbgk_link_snapshot(f->L, stage, inlink, link, links);
}

extern "C" int dbgk_fill_layout(dbgk_fill *f, uint64_t *scaf_first, dbgk_fill_item *items, dbgk_fill_gap *gaps, int32_t *repeats, char *consensus)
{
	if (!f) return DBGK_ERR_ARG;
	if (!f->resolved) return DBGK_ERR_STATE;
	if (scaf_first) memcpy(scaf_first, f->scaf_first.data(), f->scaf_first.size() * 8);
	if (items && !f->items.empty()) memcpy(items, f->items.data(), f->items.size() * sizeof(dbgk_fill_item));
	if (gaps && !f->gaps.empty()) memcpy(gaps, f->gaps.data(), f->gaps.size() * sizeof(dbgk_fill_gap));
	if (repeats && !f->repeats.empty()) memcpy(repeats, f->repeats.data(), f->repeats.size() * 4);
	if (consensus && f->cons_bytes) {
		HIPCHK(hipSetDevice(f->L->device));
		HIPCHK(hipMemcpy(consensus, f->d_cons, f->cons_bytes, hipMemcpyDeviceToHost));
	}
	return DBGK_OK;
}

extern "C" int dbgk_fill_emit(dbgk_fill *f, const char *bases, const uint64_t *offsets, uint64_t n_contigs, const dbgk_fill_item *items,
                              uint64_t n_items, char *out, uint64_t capacity, uint64_t *out_len)
{
	if (!f || (n_items && !items) || !out_len || n_items >= (1ull << 31) || n_contigs >= (1ull << 30) || !link_check_offsets(bases, offsets, n_contigs))
		return DBGK_ERR_ARG;
	std::vector<uint64_t> item_off(n_items + 1, 0);
	std::vector<fillk::EmitItem> dev_items(n_items);
	for (uint64_t t = 0; t < n_items; ++t) {
		const dbgk_fill_item &it = items[t];
		fillk::EmitItem d{0, 0, 0};
		if (it.contig >= 0) {
			if ((uint64_t)it.contig >= n_contigs || (it.reversed != 0 && it.reversed != 1)) return DBGK_ERR_ARG;
			const uint64_t len = offsets[it.contig + 1] - offsets[it.contig];
			if (it.length > len) return DBGK_ERR_ARG;
			d.kind = (uint32_t)it.reversed;
			d.src = it.reversed ? offsets[it.contig] + len - 1 : offsets[it.contig];   // (len 0: length 0, never read)
		} else {
			if (it.length && (it.cons_off > f->cons_bytes || it.length > f->cons_bytes - it.cons_off)) return DBGK_ERR_ARG;
			d.kind = 2;
			d.src = it.cons_off;
		}
		dev_items[t] = d;
		item_off[t + 1] = item_off[t] + it.length;
	}
	const uint64_t total = item_off[n_items];
	*out_len = total;
	if (!total) return DBGK_OK;
	if (!out || capacity < total) return DBGK_ERR_CAPACITY;
	dbgk_link *l = f->L;
	float ms = 0;
	auto launch = [&](const uint8_t *d_bases, const uint64_t *, const void *d_items, const uint64_t *d_ioff, uint8_t *d_out) {
		hipLaunchKernelGGL(fillk::k_fill_emit, dim3(link_grid(l, (total + 7) / 8)), dim3(fillk::kFillThreads), 0, l->stream, d_bases, f->d_cons,
		                   static_cast<const fillk::EmitItem *>(d_items), d_ioff, (uint32_t)n_items, total, d_out);
	};
	const int rc = link_run_emit(l, "dbgk_fill_emit", bases, offsets, n_contigs, false, dev_items.data(), n_items * sizeof(fillk::EmitItem), item_off, out,
	                             &ms, launch);
	if (rc) return rc;
	f->stats.ms_emit = ms;
	f->stats.emit_bytes = total;
	return DBGK_OK;
}

extern "C" int dbgk_fill_batch_stats(dbgk_fill *f, dbgk_fill_timing *out)
{
	if (!f || !out) return DBGK_ERR_ARG;
	*out = f->stats;
	return DBGK_OK;
}
