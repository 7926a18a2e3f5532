// SIMPLIFY: host side of the traced simplification paths (include/dbgk.h, SIMPLIFY section; kernels in dbgk_simplify.h and
// dbgk_wide_simplify.h).  Works on the device copy of the table a CONTIG handle holds (dbgk_host_contig.h).
//
// A trace call goes through its rows in batches.  Per batch: the length pass writes one row per request, the rows come back, the host
// scans their lengths, and the fill pass writes nodes and base codes back to back -- the device never holds requests x cutoff.  A batch
// is as many rows as fit kTraceBudget bytes of nodes and base codes if every walk ran to the cutoff (at most kTraceMaxRows); the test
// hook simplify_batch=N makes it N requests (N branching slots for dbgk_simplify_trace_branches).

namespace {

constexpr uint64_t kTraceBudget = 256ull << 20;
constexpr uint64_t kTraceMaxRows = 1ull << 20;

static_assert(sizeof(dbgk_trace_row) == 24 && sizeof(simpk::Row) == 24 && offsetof(dbgk_trace_row, direct) == 16 && offsetof(simpk::Row, direct) == 16 &&
              offsetof(dbgk_trace_row, status) == 18 && offsetof(simpk::Row, status) == 18, "dbgk_trace_row layout");
static_assert(sizeof(dbgk_trace_request) == 16 && sizeof(dbgk_trace_summary) == 32 && sizeof(dbgk_simplify_timing) == 64, "SIMPLIFY layouts");
static_assert(offsetof(dbgk_node, l_link) == 8 && offsetof(dbgk_node, r_link) == 12 && offsetof(dbgk_node32, l_link) == 16 && offsetof(dbgk_node32, r_link) == 20,
              "k_simp_update writes both link words with one 8-byte store");

contigk::Table simplify_table(const dbgk_contig *c)
{
	contigk::Table t;
	t.array = c->d_array;
	t.nul = c->d_nul;
	t.del = c->d_del;
	t.klink = c->d_klink;
	t.size = c->size;
	t.magic = make_mod_magic(c->size);
	t.k = c->p.k;
	return t;
}

wctgk::WideTable simplify_wide_table(const dbgk_contig *c)
{
	wctgk::WideTable t;
	t.array = c->d_array32;
	t.nul = c->d_nul;
	t.del = c->d_del;
	t.klink = c->d_klink;
	t.size = c->size;
	t.magic = make_mod_magic(c->size);
	t.k = c->p.k;
	return t;
}

// device time of what was queued between the two events; waits for it
int simplify_elapsed(dbgk_contig *c, double &ms)
{
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(c->ev[1], c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	float t = 0;
	HIPCHK(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
	ms += t;
	return DBGK_OK;
}

// slots: the requests' slots, or the branching slots (8 rows each); direct: the requests' directions, or a null pointer for branches
int simplify_trace(dbgk_contig *c, const std::vector<uint32_t> &slots, const std::vector<int8_t> *direct, int32_t cutoff, dbgk_trace_summary *out)
{
	using namespace simpk;
	const bool branches = direct == nullptr;
	const uint64_t per = branches ? 8 : 1, n_items = slots.size(), n_rows = n_items * per;
	HIPCHK(hipSetDevice(c->device));
	c->traced = false;
	c->trace_rows.assign(n_rows, dbgk_trace_row{});
	c->trace_first.assign(n_rows + 1, 0);
	c->trace_nodes.clear();
	c->trace_bases.clear();
	c->trace_summary = dbgk_trace_summary{};
	uint64_t batch_rows = std::min<uint64_t>(kTraceMaxRows, std::max<uint64_t>(8, kTraceBudget / (5ull * (uint64_t)std::max(cutoff, 1))));
	uint64_t batch_items = std::max<uint64_t>(1, batch_rows / per);
	if (const char *hook = dbgk_hook("simplify_batch")) batch_items = std::max<uint64_t>(1, std::min<uint64_t>(strtoull(hook, nullptr, 10), kTraceMaxRows / per));
	const contigk::Table t = simplify_table(c);
	const wctgk::WideTable wt = simplify_wide_table(c);
	const dim3 block(kSimpThreads);
	dbgk_simplify_timing &tm = c->simplify_timing;
	std::vector<uint64_t> first;
	for (uint64_t i0 = 0; i0 < n_items; i0 += batch_items) {
		const uint64_t items = std::min(batch_items, n_items - i0), rows = items * per, r0 = i0 * per;
		ContigScratch mem;
		uint32_t *d_slot = nullptr;
		int8_t *d_direct = nullptr;
		Row *d_rows = nullptr;
		uint64_t *d_first = nullptr;
		if (!mem.get(d_slot, items) || !mem.get(d_direct, items) || !mem.get(d_rows, rows) || !mem.get(d_first, rows)) return DBGK_ERR_NOMEM;
		HIPCHK(hipMemcpyAsync(d_slot, slots.data() + i0, items * 4, hipMemcpyHostToDevice, c->stream));
		if (!branches) HIPCHK(hipMemcpyAsync(d_direct, direct->data() + i0, items, hipMemcpyHostToDevice, c->stream));
		const dim3 grid(contig_grid(c, rows));
		HIPCHK(hipEventRecord(c->ev[0], c->stream));
		if (branches) {
			if (c->wide) hipLaunchKernelGGL(wsimpk::k_wsimp_branches, grid, block, 0, c->stream, wt, d_slot, (uint32_t)rows, cutoff, c->p.kmer_freq_cutoff, d_rows);
			else hipLaunchKernelGGL(k_simp_branches, grid, block, 0, c->stream, t, d_slot, (uint32_t)rows, cutoff, c->p.kmer_freq_cutoff, d_rows);
		} else {
			if (c->wide) hipLaunchKernelGGL(wsimpk::k_wsimp_trace, grid, block, 0, c->stream, wt, d_slot, d_direct, (uint32_t)rows, cutoff, d_rows);
			else hipLaunchKernelGGL(k_simp_trace, grid, block, 0, c->stream, t, d_slot, d_direct, (uint32_t)rows, cutoff, d_rows);
		}
		int rc = simplify_elapsed(c, branches ? tm.ms_branches : tm.ms_trace);
		if (rc) return rc;
		HIPCHK(hipMemcpy(c->trace_rows.data() + r0, d_rows, rows * sizeof(Row), hipMemcpyDeviceToHost));
		tm.bytes_returned += rows * sizeof(Row);
		// the batch's steps back to back
		first.assign(rows, 0);
		uint64_t steps = 0;
		const uint64_t base = c->trace_nodes.size();
		for (uint64_t i = 0; i < rows; ++i) {
			const dbgk_trace_row &r = c->trace_rows[r0 + i];
			first[i] = steps;
			c->trace_first[r0 + i] = base + steps;
			steps += r.len;
			c->trace_summary.traced += r.len ? 1 : 0;
		}
		if (steps) {
			uint32_t *d_nodes = nullptr;
			uint8_t *d_codes = nullptr;
			if (!mem.get(d_nodes, steps) || !mem.get(d_codes, steps)) return DBGK_ERR_NOMEM;
			HIPCHK(hipMemcpyAsync(d_first, first.data(), rows * 8, hipMemcpyHostToDevice, c->stream));
			HIPCHK(hipEventRecord(c->ev[0], c->stream));
			if (c->wide) hipLaunchKernelGGL(wsimpk::k_wsimp_fill, grid, block, 0, c->stream, wt, d_rows, d_first, (uint32_t)rows, cutoff, d_nodes, d_codes);
			else hipLaunchKernelGGL(k_simp_fill, grid, block, 0, c->stream, t, d_rows, d_first, (uint32_t)rows, cutoff, d_nodes, d_codes);
			rc = simplify_elapsed(c, tm.ms_fill);
			if (rc) return rc;
			c->trace_nodes.resize(base + steps);
			c->trace_bases.resize(base + steps);
			HIPCHK(hipMemcpy(c->trace_nodes.data() + base, d_nodes, steps * 4, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(c->trace_bases.data() + base, d_codes, steps, hipMemcpyDeviceToHost));
			tm.bytes_returned += steps * 5;
		}
		++c->trace_summary.batches;
		++tm.batches;
	}
	c->trace_first[n_rows] = c->trace_nodes.size();
	c->trace_summary.rows = n_rows;
	c->trace_summary.nodes = c->trace_nodes.size();
	c->traced = true;
	if (out) *out = c->trace_summary;
	return DBGK_OK;
}

} // namespace

extern "C" int dbgk_simplify_trace(dbgk_contig *c, const dbgk_trace_request *req, uint64_t n, int32_t len_cutoff, dbgk_trace_summary *out)
{
	if (!c || (n && !req) || len_cutoff > DBGK_TRACE_MAX_CUTOFF) return DBGK_ERR_ARG;
	if (!c->table_set) return DBGK_ERR_STATE;
	std::vector<uint32_t> slots(n);
	std::vector<int8_t> direct(n);
	for (uint64_t i = 0; i < n; ++i) {
		if (req[i].slot >= c->size || (req[i].direct != 1 && req[i].direct != -1) || req[i].reserved) return DBGK_ERR_ARG;
		slots[i] = (uint32_t)req[i].slot;
		direct[i] = (int8_t)req[i].direct;
	}
	return simplify_trace(c, slots, &direct, len_cutoff, out);
}

extern "C" int dbgk_simplify_trace_branches(dbgk_contig *c, const uint64_t *slots, uint64_t n, int32_t len_cutoff, dbgk_trace_summary *out)
{
	if (!c || (n && !slots) || len_cutoff > DBGK_TRACE_MAX_CUTOFF) return DBGK_ERR_ARG;
	if (!c->table_set) return DBGK_ERR_STATE;
	std::vector<uint32_t> s(n);
	for (uint64_t i = 0; i < n; ++i) {
		if (slots[i] >= c->size) return DBGK_ERR_ARG;
		s[i] = (uint32_t)slots[i];
	}
	return simplify_trace(c, s, nullptr, len_cutoff, out);
}

extern "C" int dbgk_simplify_trace_results(dbgk_contig *c, dbgk_trace_row *rows, uint64_t *node_offsets, uint32_t *nodes, uint8_t *bases)
{
	if (!c) return DBGK_ERR_ARG;
	if (!c->traced) return DBGK_ERR_STATE;
	if (rows && !c->trace_rows.empty()) memcpy(rows, c->trace_rows.data(), c->trace_rows.size() * sizeof(dbgk_trace_row));
	if (node_offsets) memcpy(node_offsets, c->trace_first.data(), c->trace_first.size() * 8);
	if (nodes && !c->trace_nodes.empty()) memcpy(nodes, c->trace_nodes.data(), c->trace_nodes.size() * 4);
	if (bases && !c->trace_bases.empty()) memcpy(bases, c->trace_bases.data(), c->trace_bases.size());
	return DBGK_OK;
}

extern "C" int dbgk_simplify_update(dbgk_contig *c, const uint64_t *slots, uint64_t n)
{
	if (!c || (n && !slots)) return DBGK_ERR_ARG;
	if (!c->table_set) return DBGK_ERR_STATE;
	std::vector<uint32_t> s(n);
	for (uint64_t i = 0; i < n; ++i) {
		if (slots[i] >= c->size) return DBGK_ERR_ARG;
		s[i] = (uint32_t)slots[i];
	}
	if (!n) return DBGK_OK;
	// no slot and no flag byte twice: nothing in the kernel writes one address from two threads
	std::sort(s.begin(), s.end());
	s.erase(std::unique(s.begin(), s.end()), s.end());
	const uint64_t m = s.size();
	std::vector<uint2> links(m);
	std::vector<uint16_t> records(m);
	std::vector<uint32_t> byte_at;
	std::vector<uint8_t> byte_val;
	for (uint64_t i = 0; i < m; ++i) {
		const uint32_t v = s[i];
		links[i] = c->wide ? make_uint2(c->h_array32[v].l_link, c->h_array32[v].r_link) : make_uint2(c->h_array[v].l_link, c->h_array[v].r_link);
		records[i] = c->h_klink[v];
		if (byte_at.empty() || byte_at.back() != v >> 3) {
			byte_at.push_back(v >> 3);
			byte_val.push_back(c->h_del[v >> 3]);
		}
	}
	const uint64_t nb = byte_at.size();
	HIPCHK(hipSetDevice(c->device));
	ContigScratch mem;
	uint32_t *d_slot = nullptr, *d_byte_at = nullptr;
	uint2 *d_links = nullptr;
	uint16_t *d_records = nullptr;
	uint8_t *d_byte_val = nullptr;
	if (!mem.get(d_slot, m) || !mem.get(d_links, m) || !mem.get(d_records, m) || !mem.get(d_byte_at, nb) || !mem.get(d_byte_val, nb)) return DBGK_ERR_NOMEM;
	HIPCHK(hipMemcpyAsync(d_slot, s.data(), m * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_links, links.data(), m * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_records, records.data(), m * 2, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_byte_at, byte_at.data(), nb * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_byte_val, byte_val.data(), nb, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipEventRecord(c->ev[0], c->stream));
	uint8_t *array = c->wide ? reinterpret_cast<uint8_t *>(c->d_array32.p) : reinterpret_cast<uint8_t *>(c->d_array.p);
	hipLaunchKernelGGL(simpk::k_simp_update, dim3(contig_grid(c, m)), dim3(simpk::kSimpThreads), 0, c->stream, array,
	                   (uint32_t)(c->wide ? sizeof(dbgk_node32) : sizeof(dbgk_node)), (uint32_t)(c->wide ? offsetof(dbgk_node32, l_link) : offsetof(dbgk_node, l_link)),
	                   c->d_klink, c->d_del, d_slot, d_links, d_records, (uint32_t)m, d_byte_at, d_byte_val, (uint32_t)nb);
	const int rc = simplify_elapsed(c, c->simplify_timing.ms_update);
	if (rc) return rc;
	c->simplify_timing.updated_slots += m;
	return DBGK_OK;
}

extern "C" int dbgk_simplify_timing_get(dbgk_contig *c, dbgk_simplify_timing *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	*out = c->simplify_timing;
	return DBGK_OK;
}
