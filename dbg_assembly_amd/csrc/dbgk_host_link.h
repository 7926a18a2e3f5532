// LINK: host side of link_scaffold on the GPU (include/dbgk.h, LINK section; kernels in dbgk_link.h).  The device builds the link
// table; the reference's clean-up passes and its walk are serial and order-dependent, O(contigs + links), and run here in its order.

struct dbgk_link : StageDev {
	dbgk_link_params p{};
	// contigs
	std::vector<uint32_t> lens;
	DevBuf<uint32_t> d_lens;
	bool contigs_set = false;
	// the entries of every batch so far, two per record, in record order; sorted in place by dbgk_link_build
	DevBuf<uint64_t> d_keys, d_vals;
	uint64_t n_entries = 0, cap_entries = 0;
	DevBuf<uint8_t> d_in;       // staging of one batch of records or hits
	DevBuf<linkk::Counters> d_ctr;
	StageEvents<2> ev;
	bool built = false;
	// the table on the host: links of node i are links[first[i] .. first[i + 1]) in chain order
	std::vector<uint64_t> first;
	std::vector<dbgk_link_entry> links;
	dbgk_link_counters counters{};
	// dbgk_link_resolve
	bool resolved = false;
	std::vector<dbgk_link_entry> snap_links[2];
	std::vector<uint8_t> snap_link[2], snap_inlink[2];
	std::vector<uint64_t> scaf_first;
	std::vector<dbgk_link_item> items;
	std::vector<int32_t> repeats;
	dbgk_link_summary summary{};
	dbgk_link_timing stats{};
};

static_assert(sizeof(dbgk_link_pair) == 32 && sizeof(linkk::Pair) == 32, "dbgk_link_pair is 32 bytes");
static_assert(offsetof(dbgk_link_pair, direct1) == 24 && offsetof(dbgk_link_pair, direct2) == 25, "dbgk_link_pair layout");
static_assert(sizeof(dbgk_link_entry) == 16 && sizeof(linkk::Entry) == 16 && offsetof(dbgk_link_entry, size) == 8, "dbgk_link_entry layout");
static_assert(sizeof(dbgk_link_item) == 8 && sizeof(linkk::Item) == 8, "dbgk_link_item layout");
static_assert(sizeof(dbgk_map_hit) == 32 && sizeof(linkk::Hit) == 32, "dbgk_map_hit layout");

extern "C" int dbgk_link_create(const dbgk_link_params *p, int device, dbgk_link **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (!p || device < 0 || (p->mate_pair != 0 && p->mate_pair != 1) || p->pair_num_cut < 0 || p->insert_size <= 0) return DBGK_ERR_ARG;
	dbgk_link *l = new (std::nothrow) dbgk_link;
	if (!l) return DBGK_ERR_NOMEM;
	l->p = *p;
	int rc = stage_open(*l, device);
	if (!rc) rc = l->ev.create();
	if (!rc) rc = l->d_ctr.reserve(sizeof(linkk::Counters));
	if (!rc && hipMemsetAsync(l->d_ctr, 0, sizeof(linkk::Counters), l->stream) != hipSuccess) rc = DBGK_ERR_HIP;
	if (rc) {
		dbgk_link_destroy(l);
		return rc;
	}
	*out = l;
	return DBGK_OK;
}

extern "C" int dbgk_link_destroy(dbgk_link *l)
{
	if (!l) return DBGK_ERR_ARG;
	stage_drain(l->device, l->stream);
	delete l;
	return DBGK_OK;
}

extern "C" int dbgk_link_set_contigs(dbgk_link *l, const uint32_t *lengths, uint64_t n_contigs)
{
	// node ids are 32 bits and 2 * n + 1 of them exist; a length takes part in the reference's int arithmetic
	if (!l || (n_contigs && !lengths) || n_contigs >= (1ull << 30)) return DBGK_ERR_ARG;
	for (uint64_t i = 0; i < n_contigs; ++i)
		if (lengths[i] >= (1u << 31)) return DBGK_ERR_ARG;
	if (l->n_entries || l->built) return DBGK_ERR_STATE;
	HIPCHK(hipSetDevice(l->device));
	l->contigs_set = false;
	l->d_lens.release();
	if (l->d_lens.reserve((n_contigs + 1) * 4)) return DBGK_ERR_NOMEM;
	if (n_contigs) HIPCHK(hipMemcpyAsync(l->d_lens, lengths, n_contigs * 4, hipMemcpyHostToDevice, l->stream));
	HIPCHK(hipStreamSynchronize(l->stream));
	l->lens.assign(lengths, lengths + n_contigs);
	l->contigs_set = true;
	return DBGK_OK;
}

// room for n_new more entries and for a batch of in_bytes
static int link_reserve(dbgk_link *l, uint64_t n_new, uint64_t in_bytes)
{
	if (l->n_entries + n_new > l->cap_entries) {
		const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(l->n_entries + n_new, 2 * l->cap_entries), 1 << 16);
		DevBuf<uint64_t> k, v;
		if (k.reserve(cap * 8) || v.reserve(cap * 8)) return DBGK_ERR_NOMEM;
		if (l->n_entries) {
			HIPCHK(hipMemcpyAsync(k, l->d_keys, l->n_entries * 8, hipMemcpyDeviceToDevice, l->stream));
			HIPCHK(hipMemcpyAsync(v, l->d_vals, l->n_entries * 8, hipMemcpyDeviceToDevice, l->stream));
			HIPCHK(hipStreamSynchronize(l->stream));
		}
		l->d_keys.take(k);
		l->d_vals.take(v);
		l->cap_entries = cap;
	}
	if (l->d_in.reserve(in_bytes, 1 << 20)) return DBGK_ERR_NOMEM;
	return DBGK_OK;
}

static unsigned link_grid(const dbgk_link *l, uint64_t n)
{
	return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + linkk::kLinkThreads - 1) / linkk::kLinkThreads, (uint64_t)l->n_cu * 8));
}

static int link_add(dbgk_link *l, const void *a, const void *b, uint64_t n, bool from_hits)
{
	// an entry's index is kept in 32 bits
	if (l->n_entries + 2 * n >= (1ull << 32)) return DBGK_ERR_CAPACITY;
	if (!l->contigs_set || l->built) return DBGK_ERR_STATE;
	if (!n) return DBGK_OK;
	HIPCHK(hipSetDevice(l->device));
	const uint64_t bytes = n * 32;
	int rc = link_reserve(l, 2 * n, from_hits ? 2 * bytes : bytes);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(l->d_in, a, bytes, hipMemcpyHostToDevice, l->stream));
	if (from_hits) HIPCHK(hipMemcpyAsync(l->d_in + bytes, b, bytes, hipMemcpyHostToDevice, l->stream));
	HIPCHK(hipEventRecord(l->ev[0], l->stream));
	const uint32_t nc = (uint32_t)l->lens.size();
	if (from_hits) {
		const linkk::Hit *h1 = reinterpret_cast<const linkk::Hit *>(l->d_in.p);
		hipLaunchKernelGGL(linkk::k_link_orient<true>, dim3(link_grid(l, n)), dim3(linkk::kLinkThreads), 0, l->stream, (const linkk::Pair *)nullptr,
		                   h1, h1 + n, n, l->d_lens, nc, l->p.mate_pair, l->p.insert_size, l->n_entries, l->d_keys, l->d_vals, l->d_ctr);
	} else {
		hipLaunchKernelGGL(linkk::k_link_orient<false>, dim3(link_grid(l, n)), dim3(linkk::kLinkThreads), 0, l->stream,
		                   reinterpret_cast<const linkk::Pair *>(l->d_in.p), (const linkk::Hit *)nullptr, (const linkk::Hit *)nullptr, n, l->d_lens, nc,
		                   l->p.mate_pair, l->p.insert_size, l->n_entries, l->d_keys, l->d_vals, l->d_ctr);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(l->ev[1], l->stream));
	HIPCHK(hipStreamSynchronize(l->stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
	l->stats.ms_orient += ms;
	l->stats.records += n;
	l->n_entries += 2 * n;
	return DBGK_OK;
}

extern "C" int dbgk_link_add_pairs(dbgk_link *l, const dbgk_link_pair *recs, uint64_t n)
{
	if (!l || (n && !recs) || n >= (1ull << 31)) return DBGK_ERR_ARG;
	const uint64_t nc = l->lens.size();
	for (uint64_t i = 0; i < n; ++i)
		if ((uint64_t)(uint32_t)recs[i].contig1 >= nc || (uint64_t)(uint32_t)recs[i].contig2 >= nc) return DBGK_ERR_ARG;
	return link_add(l, recs, nullptr, n, false);
}

extern "C" int dbgk_link_add_hits(dbgk_link *l, const dbgk_map_hit *hits1, const dbgk_map_hit *hits2, uint64_t n_pairs)
{
	if (!l || (n_pairs && (!hits1 || !hits2)) || n_pairs >= (1ull << 31)) return DBGK_ERR_ARG;
	return link_add(l, hits1, hits2, n_pairs, true);
}

extern "C" int dbgk_link_build(dbgk_link *l)
{
	if (!l) return DBGK_ERR_ARG;
	if (!l->contigs_set || l->built) return DBGK_ERR_STATE;
	HIPCHK(hipSetDevice(l->device));
	linkk::Counters hc{};
	HIPCHK(hipMemcpyAsync(&hc, l->d_ctr, sizeof hc, hipMemcpyDeviceToHost, l->stream));
	HIPCHK(hipStreamSynchronize(l->stream));
	l->counters = dbgk_link_counters{hc.cls[0], hc.cls[1], hc.cls[2], hc.cls[3], hc.cls[4]};
	const uint64_t n = l->n_entries, n_kept = 2 * hc.kept;
	const uint64_t n_nodes = 2 * l->lens.size() + 1;
	l->first.assign(n_nodes + 1, 0);
	l->links.clear();
	l->stats.kept = hc.kept;
	l->stats.entries = n_kept;
	uint64_t n_links = 0;
	if (n_kept) {
		float ms = 0;
		auto t0 = std::chrono::steady_clock::now();
		// stable, so the entries of one (source, target) stay in record order; the dropped entries end up behind position n_kept
		if (int rc = dbgk_internal_sort_pairs(l->d_keys, l->d_vals, n, l->stream)) return rc;
		l->stats.ms_sort += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		DevBuf<uint64_t> d_okeys, d_ovals;
		DevBuf<linkk::Entry> d_slots, d_out;
		DevBuf<uint32_t> d_src;
		// at most one link per kept entry
		if (d_okeys.reserve(n_kept * 8) || d_ovals.reserve(n_kept * 8) || d_slots.reserve(n_kept * 16)) return DBGK_ERR_NOMEM;
		int rc = DBGK_OK;
		auto step = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = hip_fail(e, "dbgk_link_build", __LINE__); };
		step(hipEventRecord(l->ev[0], l->stream));
		hipLaunchKernelGGL(linkk::k_link_reduce, dim3(link_grid(l, n_kept)), dim3(linkk::kLinkThreads), 0, l->stream, l->d_keys, l->d_vals, n_kept,
		                   d_okeys, d_ovals, d_slots, l->d_ctr);
		step(hipGetLastError());
		step(hipEventRecord(l->ev[1], l->stream));
		step(hipMemcpyAsync(&hc, l->d_ctr, sizeof hc, hipMemcpyDeviceToHost, l->stream));
		step(hipStreamSynchronize(l->stream));
		if (!rc) {
			step(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
			l->stats.ms_reduce += ms;
			n_links = hc.links;
		}
		if (!rc && n_links) {
			t0 = std::chrono::steady_clock::now();
			if (dbgk_internal_sort_pairs(d_okeys, d_ovals, n_links, l->stream)) rc = DBGK_ERR_HIP;
			l->stats.ms_sort += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
			if (!rc && (d_out.reserve(n_links * 16) || d_src.reserve(n_links * 4))) rc = DBGK_ERR_NOMEM;
			std::vector<uint32_t> src(n_links);
			l->links.resize(n_links);
			if (!rc) {
				step(hipEventRecord(l->ev[0], l->stream));
				hipLaunchKernelGGL(linkk::k_link_chain, dim3(link_grid(l, n_links)), dim3(linkk::kLinkThreads), 0, l->stream, d_okeys, d_ovals, n_links,
				                   d_slots, d_out, d_src);
				step(hipGetLastError());
				step(hipEventRecord(l->ev[1], l->stream));
				step(hipMemcpyAsync(l->links.data(), d_out, n_links * 16, hipMemcpyDeviceToHost, l->stream));
				step(hipMemcpyAsync(src.data(), d_src, n_links * 4, hipMemcpyDeviceToHost, l->stream));
				step(hipStreamSynchronize(l->stream));
			}
			if (!rc) {
				step(hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
				l->stats.ms_chain += ms;
				for (uint64_t j = 0; j < n_links; ++j) l->first[(uint64_t)src[j] + 1]++;
				for (uint64_t i = 0; i < n_nodes; ++i) l->first[i + 1] += l->first[i];
			}
		}
		if (rc) return rc;
	}
	l->stats.links = n_links;
	l->built = true;
	return DBGK_OK;
}

extern "C" int dbgk_link_export(dbgk_link *l, uint64_t *first, dbgk_link_entry *links, uint64_t capacity, uint64_t *n_links,
                                dbgk_link_counters *counters)
{
	if (!l || !n_links) return DBGK_ERR_ARG;
	if (!l->built) return DBGK_ERR_STATE;
	*n_links = l->links.size();
	if (counters) *counters = l->counters;
	if (first) memcpy(first, l->first.data(), l->first.size() * 8);
	if (links) {
		if (capacity < l->links.size()) return DBGK_ERR_CAPACITY;
		if (!l->links.empty()) memcpy(links, l->links.data(), l->links.size() * 16);
	}
	return DBGK_OK;
}

namespace {

// the state main() of the reference holds behind the map files
struct LinkPasses {
	const dbgk_link_params &P;
	const std::vector<uint32_t> &lens;
	const std::vector<uint64_t> &first;
	std::vector<dbgk_link_entry> e;          // ctgLink: the chains, cleared entries included
	std::vector<uint8_t> link, inlink, del;  // linkStat
	uint64_t n_nodes;
	dbgk_link_summary s{};
	std::vector<int32_t> repeat_nodes;

	LinkPasses(const dbgk_link *l)
	    : P(l->p), lens(l->lens), first(l->first), e(l->links), link(l->first.size() - 1, 0), inlink(l->first.size() - 1, 0),
	      del(l->first.size() - 1, 0), n_nodes(l->first.size() - 1) {}

	static void clear(dbgk_link_entry &x) { x.target = 0; x.freq = 0; x.size = 0; }
	static uint32_t pair_id(uint32_t id) { return id % 2 == 0 ? id - 1 : id + 1; }
	uint64_t node_len(uint32_t id) const { return id % 2 == 1 ? lens[id / 2] : 0; } // contig_seqs[even] is the empty string

	void remove_lowfreq_link_and_stat() // link_func.cpp:477-511
	{
		for (uint64_t i = 0; i < n_nodes; ++i) {
			int link_num = 0;
			for (uint64_t j = first[i]; j < first[i + 1]; ++j) {
				if ((int32_t)e[j].freq < P.pair_num_cut) {
					clear(e[j]);
					s.lowfreq++;
				} else {
					link_num++;
					if (inlink[e[j].target] < 255) inlink[e[j].target]++;
				}
			}
			if (first[i] < first[i + 1]) link[i] = (uint8_t)(link_num < 255 ? link_num : 255);
		}
	}
	// get_next_linked_id, :826-840
	uint32_t next_linked(uint32_t id, int &gap) const
	{
		for (uint64_t j = first[id]; j < first[id + 1]; ++j)
			if (e[j].freq > 0) {
				gap = (int)(e[j].size / (int64_t)e[j].freq);
				return e[j].target;
			}
		return 0;
	}
	void delete_linked_id(uint32_t source, uint32_t target) // :671-694
	{
		for (uint64_t j = first[source]; j < first[source + 1]; ++j)
			if (e[j].freq > 0 && e[j].target == target) {
				clear(e[j]);
				if (link[source] > 0) link[source]--;
				if (inlink[target] > 0) inlink[target]--;
				break;
			}
	}
	void remove_interleaving_links() // :543-581
	{
		for (uint64_t i = 1; i < n_nodes; ++i) {
			const uint32_t start = (uint32_t)i;
			if (del[start] != 0 || link[start] != 2) continue;
			uint32_t ids[2] = {0, 0};
			int gaps[2] = {0, 0}, k = 0;
			for (uint64_t j = first[start]; j < first[start + 1] && k < 2; ++j) // get_all_linked_ids: link == 2 live entries
				if (e[j].freq > 0) {
					ids[k] = e[j].target;
					gaps[k++] = (int)(e[j].size / (int64_t)e[j].freq);
				}
			for (int a = 0; a < 2; ++a) { // :553-564, then :566-577
				const int b = 1 - a;
				if (link[ids[a]] == 1 && inlink[ids[a]] == 1) {
					const uint32_t middle = ids[a] % 2 == 1 ? ids[a] : ids[a] - 1;
					const int judge_len = gaps[b] * 2;
					int end_insert = 0;
					const uint32_t end_node = next_linked(ids[a], end_insert);
					// contig_seqs[middle].size() < judge_len compares as unsigned 64-bit
					if (end_node == ids[b] && gaps[a] < judge_len && end_insert < judge_len && node_len(middle) < (uint64_t)(int64_t)judge_len) {
						delete_linked_id(start, end_node);
						s.interleave++;
					}
				}
			}
		}
	}
	void remove_repeat_nodes() // :713-726
	{
		for (uint64_t i = 1; i < n_nodes; ++i)
			if (del[i] == 0 && (inlink[i] >= 2 || link[i] >= 2)) {
				repeat_nodes.push_back((int32_t)i);
				del[i] = 1;
				del[pair_id((uint32_t)i)] = 1;
				repeat_nodes.push_back((int32_t)pair_id((uint32_t)i));
			}
		s.repeat_nodes = repeat_nodes.size() / 2;
	}
	void remove_links_from_deleted_nodes() // :747-785: a cleared entry is visited too, its target is node 0
	{
		for (uint64_t i = 0; i < n_nodes; ++i)
			for (uint64_t j = first[i]; j < first[i + 1]; ++j) {
				const uint32_t target = e[j].target;
				if (del[i] == 1 || del[target] == 1) {
					clear(e[j]);
					s.deleted++;
					if (link[i] > 0) link[i]--;
					if (inlink[target] > 0) inlink[target]--;
				}
			}
	}
	void get_linear_seq(uint32_t start, std::vector<int> &out) // :799-822
	{
		uint32_t next_id = start;
		int gap = 0;
		for (;;) {
			next_id = next_linked(next_id, gap);
			if (next_id == 0) break; // (a node with link == 1 has a live entry; the reference would read linkStat[-1] here)
			if (del[next_id] != 1) {
				out.push_back(gap);
				out.push_back((int)next_id);
			} else {
				break;
			}
			del[next_id] = 1;
			del[pair_id(next_id)] = 1;
			if (link[next_id] != 1) break;
		}
	}
};

// std::sort with `b.len < a.len` as the shipped reference program does it.  The order it leaves equal lengths in shows in the
// reference's output (its E. coli test runs have such ties) and is that of the libstdc++ it was built with: introsort whose pivot is
// the median of the first, middle and last element taken by value, partition over the whole range, ranges of up to 16 elements
// left to a final insertion sort.  Later libstdc++ versions move the median to the front instead and order some ties differently,
// so std::sort of the compiler at hand is not used here.
struct LenIdx {
	uint64_t len;
	uint64_t idx;
};
static bool link_by_len(const LenIdx &a, const LenIdx &b) { return b.len < a.len; }
static void link_linear_insert(LenIdx *v, int64_t last)
{
	const LenIdx val = v[last];
	int64_t next = last - 1;
	while (link_by_len(val, v[next])) {
		v[last] = v[next];
		last = next;
		--next;
	}
	v[last] = val;
}
static void link_insertion_sort(LenIdx *v, int64_t first, int64_t last)
{
	for (int64_t i = first + 1; i < last; ++i) {
		if (link_by_len(v[i], v[first])) {
			const LenIdx val = v[i];
			std::copy_backward(v + first, v + i, v + i + 1);
			v[first] = val;
		} else {
			link_linear_insert(v, i);
		}
	}
}
static void link_introsort(LenIdx *v, int64_t first, int64_t last, int depth)
{
	while (last - first > 16) {
		if (depth == 0) { // heap sort of the rest (std::partial_sort over the whole range)
			std::make_heap(v + first, v + last, link_by_len);
			std::sort_heap(v + first, v + last, link_by_len);
			return;
		}
		--depth;
		const LenIdx a = v[first], b = v[first + (last - first) / 2], c = v[last - 1];
		const LenIdx pivot = link_by_len(a, b) ? (link_by_len(b, c) ? b : link_by_len(a, c) ? c : a)
		                                       : (link_by_len(a, c) ? a : link_by_len(b, c) ? c : b);
		int64_t lo = first, hi = last;
		for (;;) {
			while (link_by_len(v[lo], pivot)) ++lo;
			--hi;
			while (link_by_len(pivot, v[hi])) --hi;
			if (!(lo < hi)) break;
			std::swap(v[lo], v[hi]);
			++lo;
		}
		link_introsort(v, lo, last, depth);
		last = lo;
	}
}
static void link_sort_by_len(std::vector<LenIdx> &v)
{
	const int64_t n = (int64_t)v.size();
	if (!n) return;
	int lg = 0;
	while ((n >> (lg + 1)) != 0) ++lg;
	link_introsort(v.data(), 0, n, 2 * lg);
	if (n > 16) {
		link_insertion_sort(v.data(), 0, 16);
		for (int64_t i = 16; i < n; ++i) link_linear_insert(v.data(), i);
	} else {
		link_insertion_sort(v.data(), 0, n);
	}
}

} // namespace

// n strings back to back, string i at bases[offsets[i] .. offsets[i + 1]): the offsets start at 0 and ascend, and bases is there
// when they name any
static bool link_check_offsets(const char *bases, const uint64_t *offsets, uint64_t n)
{
	if (!offsets || offsets[0] != 0) return false;
	for (uint64_t i = 0; i < n; ++i)
		if (offsets[i + 1] < offsets[i]) return false;
	return !offsets[n] || bases;
}

// the order both programs write in: the scaffolds of `order` by length, and the repeat contigs by length
static void link_layout_order(const dbgk_link *l, const LinkPasses &S, std::vector<LenIdx> &order, std::vector<int32_t> &repeats)
{
	link_sort_by_len(order);
	std::vector<LenIdx> rep;
	for (int32_t id : S.repeat_nodes)
		if (id % 2 == 1) rep.push_back(LenIdx{l->lens[id / 2], (uint64_t)(id / 2)});
	link_sort_by_len(rep);
	repeats.clear();
	for (const LenIdx &r : rep) repeats.push_back((int32_t)r.idx);
}

// the reference's passes over a copy of the table, the two snapshots, and its walk: per scaffold the combined list node, gap, node,
// ... (read_out_scaffold, link_scaffold.cpp:317-357; read_out_scaffinfo, link_contig.cpp:676-726).  link_contig runs no
// interleaving pass (interleave false).
static void link_passes_and_walk(dbgk_link *l, bool interleave, LinkPasses &S, std::vector<std::vector<int>> &combs)
{
	S.remove_lowfreq_link_and_stat();
	l->snap_links[0] = S.e; l->snap_link[0] = S.link; l->snap_inlink[0] = S.inlink;
	if (interleave) S.remove_interleaving_links();
	S.remove_repeat_nodes();
	S.remove_links_from_deleted_nodes();
	l->snap_links[1] = S.e; l->snap_link[1] = S.link; l->snap_inlink[1] = S.inlink;
	for (uint64_t i = 1; i < S.n_nodes; i += 2) {
		if (S.del[i] == 1) continue;
		S.del[i] = 1;
		S.del[i + 1] = 1;
		std::vector<int> right, left, comb;
		if (S.link[i] == 1) S.get_linear_seq((uint32_t)i, right);
		if (S.link[i + 1] == 1) {
			S.get_linear_seq((uint32_t)i + 1, left);
			std::reverse(left.begin(), left.end());
			for (size_t k = 0; k < left.size(); k += 2) left[k] = (int)LinkPasses::pair_id((uint32_t)left[k]);
		}
		comb = left;
		comb.push_back((int)i);
		comb.insert(comb.end(), right.begin(), right.end());
		combs.push_back(std::move(comb));
	}
}

extern "C" int dbgk_link_resolve(dbgk_link *l, dbgk_link_summary *out)
{
	if (!l || !out) return DBGK_ERR_ARG;
	if (!l->built) return DBGK_ERR_STATE;
	if (!l->resolved) {
		LinkPasses S(l);
		std::vector<std::vector<int>> combs;
		link_passes_and_walk(l, true, S, combs);
		// generate_scaffold (link_scaffold.cpp:427-463)
		std::vector<std::vector<dbgk_link_item>> scaf;
		std::vector<LenIdx> order;
		for (const std::vector<int> &comb : combs) {
			std::vector<dbgk_link_item> items;
			uint64_t len = 0;
			for (size_t k = 0; k < comb.size(); ++k) {
				if (k % 2 == 0) {
					const int id = comb[k];
					const int32_t c = id % 2 == 1 ? id / 2 : (id - 1) / 2;
					items.push_back(dbgk_link_item{c, id % 2 == 1 ? 0 : 1});
					len += l->lens[c];
				} else {
					const int gap = comb[k] > 1 ? comb[k] : 1; // the smallest gap written is 1
					items.push_back(dbgk_link_item{-1, gap});
					len += (uint64_t)gap;
				}
			}
			// scaf_len is an int in the reference; LenAndSeq.len takes it as uint64_t
			order.push_back(LenIdx{(uint64_t)(int64_t)(int)len, scaf.size()});
			scaf.push_back(std::move(items));
		}
		link_layout_order(l, S, order, l->repeats);
		l->scaf_first.assign(1, 0);
		l->items.clear();
		for (const LenIdx &o : order) {
			l->items.insert(l->items.end(), scaf[o.idx].begin(), scaf[o.idx].end());
			l->scaf_first.push_back(l->items.size());
		}
		S.s.scaffolds = scaf.size();
		S.s.items = l->items.size();
		l->summary = S.s;
		l->resolved = true;
	}
	*out = l->summary;
	return DBGK_OK;
}

extern "C" int dbgk_link_snapshot(dbgk_link *l, int32_t stage, uint8_t *inlink, uint8_t *link, dbgk_link_entry *links)
{
	if (!l || stage < 0 || stage > 1) return DBGK_ERR_ARG;
	if (!l->resolved) return DBGK_ERR_STATE;
	if (inlink) memcpy(inlink, l->snap_inlink[stage].data(), l->snap_inlink[stage].size());
	if (link) memcpy(link, l->snap_link[stage].data(), l->snap_link[stage].size());
	if (links && !l->snap_links[stage].empty()) memcpy(links, l->snap_links[stage].data(), l->snap_links[stage].size() * 16);
	return DBGK_OK;
}

extern "C" int dbgk_link_layout(dbgk_link *l, uint64_t *scaf_first, dbgk_link_item *items, int32_t *repeats)
{
	if (!l) return DBGK_ERR_ARG;
	if (!l->resolved) return DBGK_ERR_STATE;
	if (scaf_first) memcpy(scaf_first, l->scaf_first.data(), l->scaf_first.size() * 8);
	if (items && !l->items.empty()) memcpy(items, l->items.data(), l->items.size() * 8);
	if (repeats && !l->repeats.empty()) memcpy(repeats, l->repeats.data(), l->repeats.size() * 4);
	return DBGK_OK;
}

// the device side of dbgk_link_emit and dbgk_fill_emit (`who`) once the items are checked: the contig bases, the items as the
// stage's kernel reads them (item_bytes of them) and their offsets in the output go up, the contig offsets too when the kernel reads
// them (with_contig_off); launch(d_bases, d_contig_off, d_items, d_item_off, d_out) starts the kernel; the item_off.back() bytes
// it writes come down into out, and ms takes its time.
template <class Launch>
static int link_run_emit(dbgk_link *l, const char *who, const char *bases, const uint64_t *offsets, uint64_t n_contigs, bool with_contig_off,
                         const void *items, uint64_t item_bytes, const std::vector<uint64_t> &item_off, char *out, float *ms, Launch launch)
{
	const uint64_t nb = offsets[n_contigs], total = item_off.back();
	HIPCHK(hipSetDevice(l->device));
	DevBuf<uint8_t> d_bases, d_out, d_items;
	DevBuf<uint64_t> d_coff, d_ioff;
	if (d_bases.reserve(nb + 16) || d_out.reserve(((total + 7) & ~7ull) + 16) || (with_contig_off && d_coff.reserve((n_contigs + 1) * 8)) ||
	    d_ioff.reserve(item_off.size() * 8) || d_items.reserve(item_bytes))
		return DBGK_ERR_NOMEM;
	int rc = DBGK_OK;
	auto step = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = hip_fail(e, who, __LINE__); };
	if (nb) step(hipMemcpyAsync(d_bases, bases, nb, hipMemcpyHostToDevice, l->stream));
	if (with_contig_off) step(hipMemcpyAsync(d_coff, offsets, (n_contigs + 1) * 8, hipMemcpyHostToDevice, l->stream));
	step(hipMemcpyAsync(d_ioff, item_off.data(), item_off.size() * 8, hipMemcpyHostToDevice, l->stream));
	step(hipMemcpyAsync(d_items, items, item_bytes, hipMemcpyHostToDevice, l->stream));
	step(hipEventRecord(l->ev[0], l->stream));
	if (!rc) {
		launch(d_bases, d_coff, d_items, d_ioff, d_out);
		step(hipGetLastError());
	}
	step(hipEventRecord(l->ev[1], l->stream));
	step(hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, l->stream));
	step(hipStreamSynchronize(l->stream));
	if (!rc) step(hipEventElapsedTime(ms, l->ev[0], l->ev[1]));
	return rc;
}

extern "C" int dbgk_link_emit(dbgk_link *l, const char *bases, const uint64_t *offsets, uint64_t n_contigs, const dbgk_link_item *items,
                              uint64_t n_items, char *out, uint64_t capacity, uint64_t *out_len)
{
	if (!l || (n_items && !items) || !out_len || n_items >= (1ull << 31) || n_contigs >= (1ull << 30) || !link_check_offsets(bases, offsets, n_contigs))
		return DBGK_ERR_ARG;
	std::vector<uint64_t> item_off(n_items + 1, 0);
	for (uint64_t t = 0; t < n_items; ++t) {
		uint64_t len;
		if (items[t].contig >= 0) {
			if ((uint64_t)items[t].contig >= n_contigs || (items[t].value != 0 && items[t].value != 1)) return DBGK_ERR_ARG;
			len = offsets[items[t].contig + 1] - offsets[items[t].contig];
		} else {
			if (items[t].value < 0) return DBGK_ERR_ARG;
			len = (uint64_t)items[t].value;
		}
		item_off[t + 1] = item_off[t] + len;
	}
	const uint64_t total = item_off[n_items];
	*out_len = total;
	if (!total) return DBGK_OK;
	if (!out || capacity < total) return DBGK_ERR_CAPACITY;
	float ms = 0;
	auto launch = [&](const uint8_t *d_bases, const uint64_t *d_coff, const void *d_items, const uint64_t *d_ioff, uint8_t *d_out) {
		hipLaunchKernelGGL(linkk::k_link_emit, dim3(link_grid(l, (total + 7) / 8)), dim3(linkk::kLinkThreads), 0, l->stream, d_bases, d_coff,
		                   static_cast<const linkk::Item *>(d_items), d_ioff, (uint32_t)n_items, total, d_out);
	};
	const int rc = link_run_emit(l, "dbgk_link_emit", bases, offsets, n_contigs, true, items, n_items * 8, item_off, out, &ms, launch);
	if (rc) return rc;
	l->stats.ms_emit = ms;
	l->stats.emit_bytes = total;
	return DBGK_OK;
}

extern "C" int dbgk_link_batch_stats(dbgk_link *l, dbgk_link_timing *out)
{
	if (!l || !out) return DBGK_ERR_ARG;
	*out = l->stats;
	return DBGK_OK;
}
