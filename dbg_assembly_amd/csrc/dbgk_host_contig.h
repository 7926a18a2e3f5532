// CONTIG: host side of the contig read-out on the GPU (include/dbgk.h, CONTIG section; kernels in dbgk_contig.h).  The device numbers
// the live linear nodes, finds successors, checks order-independence, ranks the chains and writes the contigs; the two ordered
// compactions scan their per-tile counts on the host (a few thousand numbers).  Chains the kernels hand over are walked here, the way
// get_linear_seq does (DBG_contig/contig.cpp:832-896), in ascending slot order.
//
// A handle made by dbgk_wide_contig_create holds a table of 32-byte nodes (k up to 63, 128-bit keys; PARITY UNPINNED above k = 32, see
// dbgk_wide_contig.h): the two kernels that read keys are the wide ones, everything else -- the other eight kernels, the scans, the
// merge -- is the same code.  The host walker works on 128-bit keys for both kinds; a 16-byte node's key has the high word 0, where
// every rule of include/dbgk_wide.h is the reference's.

struct dbgk_contig : StageDev {
	StageEvents<2> ev;
	dbgk_contig_params p{};
	// the table: borrowed host arrays and their device copies
	uint64_t size = 0;
	bool wide = false;                       // 32-byte nodes: h_array32 / d_array32 instead of h_array / d_array
	const dbgk_node *h_array = nullptr;
	const dbgk_node32 *h_array32 = nullptr;
	DevBuf<dbgk_node32> d_array32;
	const uint8_t *h_nul = nullptr, *h_del = nullptr;
	const uint16_t *h_klink = nullptr;
	DevBuf<Node> d_array;
	DevBuf<uint8_t> d_nul, d_del;
	DevBuf<uint16_t> d_klink;
	bool table_set = false, done = false;
	// the kernels' contigs, back to back on the device
	DevBuf<uint8_t> d_bases, d_depths;
	// all contigs in scan order
	std::vector<uint64_t> offsets;
	std::vector<dbgk_contig_record> records;
	std::vector<char> bases, depths;
	dbgk_contig_summary summary{};
	dbgk_contig_timing timing{};
	// SIMPLIFY (dbgk_host_simplify.h): what the last trace call found
	bool traced = false;
	std::vector<dbgk_trace_row> trace_rows;
	std::vector<uint64_t> trace_first;
	std::vector<uint32_t> trace_nodes;
	std::vector<uint8_t> trace_bases;
	dbgk_trace_summary trace_summary{};
	dbgk_simplify_timing simplify_timing{};
	// ALIGN (dbgk_host_align.h): what the last dbgk_align_pairs found
	bool aligned = false;
	std::vector<dbgk_align_row> align_rows;
	std::vector<uint64_t> align_first;
	std::vector<char> align_i, align_j;
	dbgk_align_summary align_summary{};
	dbgk_align_timing align_timing{};
};

static_assert(sizeof(dbgk_contig_record) == 48 && sizeof(contigk::Record) == 48 && offsetof(dbgk_contig_record, left_mark) == 40 &&
              offsetof(contigk::Record, left_mark) == 40 && offsetof(dbgk_contig_record, mid_depth) == 45, "dbgk_contig_record layout");
static_assert(sizeof(dbgk_contig_summary) == 64 && sizeof(dbgk_contig_timing) == 88 && sizeof(contigk::PortState) == 16, "CONTIG layouts");

static int contig_create(const dbgk_contig_params *p, int device, int k_max, dbgk_contig **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (!p || device < 0 || p->k < 1 || p->k > k_max || p->kmer_freq_cutoff < 0 || p->reserved) return DBGK_ERR_ARG;
	dbgk_contig *c = new (std::nothrow) dbgk_contig;
	if (!c) return DBGK_ERR_NOMEM;
	c->p = *p;
	c->wide = k_max > 31;
	int rc = stage_open(*c, device);
	if (!rc) rc = c->ev.create();
	if (rc) {
		dbgk_contig_destroy(c);
		return rc;
	}
	*out = c;
	return DBGK_OK;
}

extern "C" int dbgk_contig_create(const dbgk_contig_params *p, int device, dbgk_contig **out) { return contig_create(p, device, 31, out); }

extern "C" int dbgk_wide_contig_create(const dbgk_contig_params *p, int device, dbgk_contig **out) { return contig_create(p, device, 63, out); }

static void contig_free_table(dbgk_contig *c)
{
	c->d_array.release(); c->d_array32.release(); c->d_nul.release(); c->d_del.release(); c->d_klink.release();
	c->d_bases.release(); c->d_depths.release();
	c->table_set = c->done = false;
}

extern "C" int dbgk_contig_destroy(dbgk_contig *c)
{
	if (!c) return DBGK_ERR_ARG;
	stage_drain(c->device, c->stream);
	delete c;
	return DBGK_OK;
}

// array: `size` nodes of node_bytes bytes each (16: dbgk_node, 32: dbgk_node32), as the handle's kind has them
static int contig_set_table(dbgk_contig *c, uint64_t size, const void *array, size_t node_bytes, const uint8_t *nul_flag, const uint8_t *del_flag,
                            const uint16_t *klink)
{
	// slots and ports are 32-bit on the device, 0xffffffff is "none"
	if (!c || !array || !nul_flag || !del_flag || !klink || size < 2 || size >= 0xffffffffull) return DBGK_ERR_ARG;
	if (c->wide != (node_bytes == sizeof(dbgk_node32))) {
		g_last_error = c->wide ? "a wide contig handle takes its table through dbgk_wide_contig_set_table" : "dbgk_wide_contig_set_table needs a handle of dbgk_wide_contig_create";
		return DBGK_ERR_STATE;
	}
	HIPCHK(hipSetDevice(c->device));
	contig_free_table(c);
	const uint64_t flag_bytes = size / 8 + 1;
	if ((c->wide ? c->d_array32.reserve(size * node_bytes) : c->d_array.reserve(size * node_bytes)) || c->d_nul.reserve(flag_bytes) ||
	    c->d_del.reserve(flag_bytes) || c->d_klink.reserve(size * 2)) {
		contig_free_table(c);
		return DBGK_ERR_NOMEM;
	}
	void *d_nodes = c->wide ? (void *)c->d_array32.p : (void *)c->d_array.p;
	const auto t0 = std::chrono::steady_clock::now();
	HIPCHK(hipMemcpyAsync(d_nodes, array, size * node_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->d_nul, nul_flag, flag_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->d_del, del_flag, flag_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->d_klink, klink, size * 2, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->timing = dbgk_contig_timing{};
	c->simplify_timing = dbgk_simplify_timing{};
	c->traced = false;
	c->timing.ms_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	c->timing.upload_bytes = size * (node_bytes + 2) + 2 * flag_bytes;
	c->size = size;
	c->h_array = c->wide ? nullptr : static_cast<const dbgk_node *>(array);
	c->h_array32 = c->wide ? static_cast<const dbgk_node32 *>(array) : nullptr;
	c->h_nul = nul_flag;
	c->h_del = del_flag;
	c->h_klink = klink;
	c->table_set = true;
	return DBGK_OK;
}

extern "C" int dbgk_contig_set_table(dbgk_contig *c, uint64_t size, const dbgk_node *array, const uint8_t *nul_flag, const uint8_t *del_flag,
                                     const uint16_t *klink)
{
	return contig_set_table(c, size, array, sizeof(dbgk_node), nul_flag, del_flag, klink);
}

extern "C" int dbgk_wide_contig_set_table(dbgk_contig *c, uint64_t size, const dbgk_node32 *array, const uint8_t *nul_flag, const uint8_t *del_flag,
                                          const uint16_t *klink)
{
	return contig_set_table(c, size, array, sizeof(dbgk_node32), nul_flag, del_flag, klink);
}

namespace {

// the reference's walk on the host table, with the delete flags of the chains walked so far.  Keys are 128-bit: a 16-byte node's has
// the high word 0, where revcomp, the comparison and hash128 of include/dbgk_wide.h are the reference's 64-bit rules
struct ContigHostWalker {
	using Key128 = dbgk_wide::Key128;
	const dbgk_node *array;          // one of the two is set
	const dbgk_node32 *array32;
	const uint8_t *nul;
	std::vector<uint8_t> del;
	const uint16_t *klink;
	uint64_t size;
	int k;

	static bool bit(const uint8_t *f, uint64_t i) { return (f[i >> 3] & (0x80u >> (i & 7u))) != 0; }
	Key128 key_at(uint64_t slot) const { return array32 ? Key128{array32[slot].kmer_hi, array32[slot].kmer_lo} : Key128{0, array[slot].kmer}; }
	uint32_t link_at(uint64_t slot, bool right) const
	{
		return array32 ? (right ? array32[slot].r_link : array32[slot].l_link) : (right ? array[slot].r_link : array[slot].l_link);
	}
	// the two steps of contig.h:119-130; the mask has 2 k - 64 bits in hi, the leftward base lands in hi from k = 33 on
	Key128 rightward(Key128 x, uint32_t base) const
	{
		Key128 r{(x.hi << 2) | (x.lo >> 62), (x.lo << 2) | base};
		const int bits = 2 * k;
		if (bits > 64) r.hi &= (1ull << (bits - 64)) - 1;
		else {
			r.hi = 0;
			if (bits < 64) r.lo &= (1ull << bits) - 1;
		}
		return r;
	}
	Key128 leftward(Key128 x, uint32_t base) const
	{
		Key128 r{x.hi >> 2, (x.lo >> 2) | (x.hi << 62)};
		const int sh = 2 * (k - 1);
		if (sh >= 64) r.hi += (uint64_t)base << (sh - 64);
		else r.lo += (uint64_t)base << sh;
		return r;
	}
	uint64_t exist(Key128 key) const   // exist_kmerset, kmerSet.cpp:280-302
	{
		uint64_t slot = dbgk_wide::hash128(key) % size;
		for (uint64_t tries = 0; tries < size; ++tries) {
			if (!bit(nul, slot)) return size;
			const Key128 at = key_at(slot);
			if (at.hi == key.hi && at.lo == key.lo) return bit(del.data(), slot) ? size : slot;
			slot = slot + 1 == size ? 0 : slot + 1;
		}
		return size;
	}
	std::string text(uint64_t slot) const   // the node's k bases
	{
		static const char fwd[] = "ACGT";
		const Key128 x = key_at(slot);
		std::string s(k, 'A');
		for (int j = 0; j < k; ++j) {
			const int sh = 2 * (k - 1 - j);
			s[j] = fwd[(sh >= 64 ? x.hi >> (sh - 64) : x.lo >> sh) & 3u];
		}
		return s;
	}
	// get_linear_seq, contig.cpp:832-896; a walk that steps to a missing k-mer ends as break before klink is looked at
	void walk(uint64_t idx, int dir, uint32_t &len, uint32_t &depth, std::string &seq, std::string &depths, uint64_t &last, uint8_t &mark,
	          uint8_t &repeat)
	{
		static const char fwd[] = "ACGT", cmp[] = "TGCA";
		const int original = dir;
		len = depth = 0;
		mark = repeat = 0;
		for (;;) {
			++len;
			const uint32_t kl = klink[idx];
			const uint32_t base = dir == 1 ? (kl >> 6) & 3u : (kl >> 2) & 3u;
			const uint32_t link = link_at(idx, dir == 1);
			uint32_t d = (link >> ((3u - base) * 8u)) & 0xffu;
			depth += d;
			if (d == 10 || d == 62) --d;
			depths.push_back((char)d);
			seq.push_back((original == dir) ? fwd[base] : cmp[base]);
			const Key128 nk = dir == 1 ? rightward(key_at(idx), base) : leftward(key_at(idx), base);
			const Key128 rc = dbgk_wide::revcomp(nk, k);
			Key128 key = nk;
			if (dbgk_wide::less_equal(rc, nk)) {   // !(nk < rc), contig.cpp:802
				key = rc;
				dir = -dir;
			}
			idx = exist(key);
			if (idx == size) {
				last = size;
				return;
			}
			const uint32_t kv = klink[idx];
			if (!(kv & 0x100u)) {
				last = idx;
				const uint32_t vl = kv & 3u, vr = (kv >> 4) & 3u;
				if (vl != 0 && vr != 0) {
					mark = 1;
					repeat = ((dir == 1 && vr > 1) || (dir == -1 && vl > 1)) ? 2 : 1;
				}
				return;
			}
			del[idx >> 3] |= (uint8_t)(0x80u >> (idx & 7u));
		}
	}
};

struct ContigScratch {   // device allocations of one read-out
	std::vector<void *> ptrs;
	template <typename T> bool get(T *&p, uint64_t n)
	{
		void *v = nullptr;
		if (hipMalloc(&v, (n ? n : 1) * sizeof(T)) != hipSuccess) return false;
		ptrs.push_back(v);
		p = static_cast<T *>(v);
		return true;
	}
	~ContigScratch()
	{
		for (void *p : ptrs) (void)hipFree(p);
	}
};

unsigned contig_grid(const dbgk_contig *c, uint64_t n)
{
	const uint64_t blocks = (n + contigk::kContigThreads - 1) / contigk::kContigThreads;
	return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)c->n_cu * 8));
}

} // namespace

extern "C" int dbgk_contig_read_out(dbgk_contig *c, dbgk_contig_summary *out)
{
	using namespace contigk;
	if (!c) return DBGK_ERR_ARG;
	if (!c->table_set) return DBGK_ERR_STATE;
	HIPCHK(hipSetDevice(c->device));
	c->d_bases.release(); c->d_depths.release();
	c->done = false;
	c->offsets.assign(1, 0);
	c->records.clear();
	c->bases.clear();
	c->depths.clear();
	c->summary = dbgk_contig_summary{};
	dbgk_contig_timing &tm = c->timing;
	tm.ms_compact = tm.ms_successors = tm.ms_mutual = tm.ms_rank = tm.ms_place = tm.ms_scatter = tm.ms_emit = tm.ms_host_walk = 0;
	tm.emit_bytes = 0;

	int rc = DBGK_OK;
	auto step = [&](hipError_t e, int line) { if (e != hipSuccess && !rc) rc = hip_fail(e, "dbgk_contig_read_out", line); };
#define CTG_STEP(expr) step((expr), __LINE__)
	auto begin = [&]() { CTG_STEP(hipEventRecord(c->ev[0], c->stream)); };
	auto end = [&](double &ms) {           // device time of what was queued since begin(); waits for it.  Every caller returns
	                                       // when rc is set: nothing more is queued on a device that has reported an error
		CTG_STEP(hipGetLastError());
		CTG_STEP(hipEventRecord(c->ev[1], c->stream));
		CTG_STEP(hipStreamSynchronize(c->stream));
		float t = 0;
		if (!rc) CTG_STEP(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
		ms += t;
	};
	const dim3 block(kContigThreads);
	ContigScratch mem;
	Table t;
	t.array = c->d_array;                // not read on a wide handle: the kernels that take a Table there read flags and link records only
	t.nul = c->d_nul;
	t.del = c->d_del;
	t.klink = c->d_klink;
	t.size = c->size;
	t.magic = make_mod_magic(c->size);
	t.k = c->p.k;
	wctgk::WideTable wt;
	wt.array = c->d_array32;
	wt.nul = c->d_nul;
	wt.del = c->d_del;
	wt.klink = c->d_klink;
	wt.size = c->size;
	wt.magic = t.magic;
	wt.k = c->p.k;

	// the live linear nodes in slot order
	const uint64_t n_tiles = (c->size + kScanTile - 1) / kScanTile;
	uint32_t *d_tile = nullptr, *d_dense_of = nullptr, *d_slot_of = nullptr;
	if (!mem.get(d_tile, n_tiles) || !mem.get(d_dense_of, c->size)) return DBGK_ERR_NOMEM;
	std::vector<uint32_t> tile(n_tiles);
	begin();
	hipLaunchKernelGGL(k_contig_count_linear, dim3((unsigned)n_tiles), block, 0, c->stream, t, d_tile);
	end(tm.ms_compact);
	if (rc) return rc;
	CTG_STEP(hipMemcpy(tile.data(), d_tile, n_tiles * 4, hipMemcpyDeviceToHost));
	if (rc) return rc;
	uint64_t n_nodes = 0;
	for (uint64_t i = 0; i < n_tiles; ++i) {
		const uint32_t n = tile[i];
		tile[i] = (uint32_t)n_nodes;
		n_nodes += n;
		if (n_nodes >= (1ull << 30)) return DBGK_ERR_ARG;
	}
	c->summary.linear_nodes = n_nodes;
	if (n_nodes == 0) {
		c->done = true;
		if (out) *out = c->summary;
		return DBGK_OK;
	}
	if (!mem.get(d_slot_of, n_nodes)) return DBGK_ERR_NOMEM;
	CTG_STEP(hipMemcpy(d_tile, tile.data(), n_tiles * 4, hipMemcpyHostToDevice));
	begin();
	hipLaunchKernelGGL(k_contig_compact_linear, dim3((unsigned)n_tiles), block, 0, c->stream, t, d_tile, d_slot_of, d_dense_of);
	end(tm.ms_compact);
	if (rc) return rc;

	// successors, order-independence, ranks
	const uint32_t n_ports = (uint32_t)(2 * n_nodes);
	uint32_t *d_raw = nullptr, *d_next = nullptr, *d_step = nullptr, *d_end = nullptr, *d_mark = nullptr;
	PortState *d_st[2] = {nullptr, nullptr};
	if (!mem.get(d_raw, n_ports) || !mem.get(d_next, n_ports) || !mem.get(d_step, n_ports) || !mem.get(d_end, n_ports) ||
	    !mem.get(d_mark, n_nodes) || !mem.get(d_st[0], n_ports) || !mem.get(d_st[1], n_ports))
		return DBGK_ERR_NOMEM;
	const dim3 pgrid(contig_grid(c, n_ports)), ngrid(contig_grid(c, n_nodes));
	begin();
	if (c->wide) hipLaunchKernelGGL(wctgk::k_wctg_successors, pgrid, block, 0, c->stream, wt, d_slot_of, d_dense_of, n_ports, d_raw, d_step, d_end);
	else hipLaunchKernelGGL(k_contig_successors, pgrid, block, 0, c->stream, t, d_slot_of, d_dense_of, n_ports, d_raw, d_step, d_end);
	end(tm.ms_successors);
	if (rc) return rc;
	begin();
	CTG_STEP(hipMemsetAsync(d_mark, 0, n_nodes * 4, c->stream));
	hipLaunchKernelGGL(k_contig_mutual, pgrid, block, 0, c->stream, d_raw, n_ports, d_next, d_mark);
	hipLaunchKernelGGL(k_contig_rank_init, pgrid, block, 0, c->stream, d_next, d_mark, d_step, n_ports, d_st[0]);
	end(tm.ms_mutual);
	if (rc) return rc;
	// a chain of m nodes is done after ceil(log2 m) rounds; after rounds with 2^rounds > n_nodes only cycles still point somewhere
	uint32_t rounds = 1;
	while ((1ull << rounds) <= n_nodes) ++rounds;
	int cur = 0;
	begin();
	for (uint32_t r = 0; r < rounds; ++r, cur ^= 1)
		hipLaunchKernelGGL(k_contig_jump, pgrid, block, 0, c->stream, d_st[cur], n_ports, d_st[cur ^ 1]);
	end(tm.ms_rank);
	if (rc) return rc;
	c->summary.rounds = rounds;
	const PortState *d_state = d_st[cur];

	// anchors, contig numbers and offsets
	const uint64_t n_tiles2 = (n_nodes + kScanTile - 1) / kScanTile;
	uint32_t *d_alen = nullptr, *d_tc = nullptr, *d_contig_of = nullptr;
	uint8_t *d_host = nullptr;
	uint64_t *d_tb = nullptr;
	if (!mem.get(d_alen, n_nodes) || !mem.get(d_host, n_nodes) || !mem.get(d_tc, n_tiles2) || !mem.get(d_tb, n_tiles2) ||
	    !mem.get(d_contig_of, n_nodes))
		return DBGK_ERR_NOMEM;
	begin();
	hipLaunchKernelGGL(k_contig_classify, dim3((unsigned)n_tiles2), block, 0, c->stream, d_state, (uint32_t)n_nodes, t.k, d_alen, d_host, d_tc, d_tb);
	end(tm.ms_place);
	if (rc) return rc;
	std::vector<uint32_t> tc(n_tiles2);
	std::vector<uint64_t> tb(n_tiles2);
	CTG_STEP(hipMemcpy(tc.data(), d_tc, n_tiles2 * 4, hipMemcpyDeviceToHost));
	CTG_STEP(hipMemcpy(tb.data(), d_tb, n_tiles2 * 8, hipMemcpyDeviceToHost));
	if (rc) return rc;
	uint64_t n_kernel = 0, total = 0;
	for (uint64_t i = 0; i < n_tiles2; ++i) {
		const uint32_t n = tc[i];
		const uint64_t b = tb[i];
		tc[i] = (uint32_t)n_kernel;
		tb[i] = total;
		n_kernel += n;
		total += b;
	}
	std::vector<uint64_t> k_off(n_kernel + 1, 0);
	std::vector<dbgk_contig_record> k_rec(n_kernel);
	std::vector<char> k_bases(total), k_depths(total);
	if (n_kernel) {
		uint64_t *d_off = nullptr;
		Record *d_rec = nullptr;
		uint16_t *d_stage = nullptr;
		if (!mem.get(d_off, n_kernel + 1) || !mem.get(d_rec, n_kernel) || !mem.get(d_stage, total)) return DBGK_ERR_NOMEM;
		if (c->d_bases.reserve(total + 8) || c->d_depths.reserve(total + 8)) return DBGK_ERR_NOMEM;
		CTG_STEP(hipMemcpy(d_tc, tc.data(), n_tiles2 * 4, hipMemcpyHostToDevice));
		CTG_STEP(hipMemcpy(d_tb, tb.data(), n_tiles2 * 8, hipMemcpyHostToDevice));
		CTG_STEP(hipMemcpy(d_off + n_kernel, &total, 8, hipMemcpyHostToDevice));
		begin();
		hipLaunchKernelGGL(k_contig_place, dim3((unsigned)n_tiles2), block, 0, c->stream, d_state, d_alen, d_slot_of, (uint32_t)n_nodes, d_tc, d_tb,
		                   d_contig_of, d_off, d_rec);
		end(tm.ms_place);
		if (rc) return rc;
		begin();
		hipLaunchKernelGGL(k_contig_scatter, ngrid, block, 0, c->stream, d_state, d_step, d_end, d_host, d_contig_of, d_off, (uint32_t)n_nodes, t.k,
		                   c->size, d_stage, d_rec);
		end(tm.ms_scatter);
		if (rc) return rc;
		begin();
		if (c->wide)
			hipLaunchKernelGGL(wctgk::k_wctg_emit, dim3(contig_grid(c, (total + 7) / 8)), block, 0, c->stream, d_stage, d_off, d_rec, c->d_array32,
			                   (uint32_t)n_kernel, total, t.k, c->d_bases, c->d_depths);
		else
			hipLaunchKernelGGL(k_contig_emit, dim3(contig_grid(c, (total + 7) / 8)), block, 0, c->stream, d_stage, d_off, d_rec, c->d_array,
			                   (uint32_t)n_kernel, total, t.k, c->d_bases, c->d_depths);
		end(tm.ms_emit);
		if (rc) return rc;
		tm.emit_bytes = 2 * total;
		CTG_STEP(hipMemcpy(k_off.data(), d_off, (n_kernel + 1) * 8, hipMemcpyDeviceToHost));
		CTG_STEP(hipMemcpy(k_rec.data(), d_rec, n_kernel * sizeof(Record), hipMemcpyDeviceToHost));
		CTG_STEP(hipMemcpy(k_bases.data(), c->d_bases, total, hipMemcpyDeviceToHost));
		CTG_STEP(hipMemcpy(k_depths.data(), c->d_depths, total, hipMemcpyDeviceToHost));
	}
	std::vector<uint8_t> host_flag(n_nodes);
	std::vector<uint32_t> slot_of(n_nodes);
	CTG_STEP(hipMemcpy(host_flag.data(), d_host, n_nodes, hipMemcpyDeviceToHost));
	CTG_STEP(hipMemcpy(slot_of.data(), d_slot_of, n_nodes * 4, hipMemcpyDeviceToHost));
	if (rc) return rc;
#undef CTG_STEP

	// the chains handed over: read_out_contig's loop (contig.cpp:930-1011) over their nodes, in slot order
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<dbgk_contig_record> h_rec;
	std::vector<std::string> h_bases, h_depths;
	uint64_t host_nodes = 0;
	for (uint64_t i = 0; i < n_nodes; ++i) host_nodes += host_flag[i];
	if (host_nodes) {
		ContigHostWalker w{c->h_array, c->h_array32, c->h_nul, std::vector<uint8_t>(c->h_del, c->h_del + c->size / 8 + 1), c->h_klink, c->size, c->p.k};
		for (uint64_t i = 0; i < n_nodes; ++i) {
			const uint64_t slot = slot_of[i];
			if (!host_flag[i] || ContigHostWalker::bit(w.del.data(), slot)) continue;
			dbgk_contig_record r{};
			std::string right, right_d, left, left_d;
			r.anchor = slot;
			r.host_walked = 1;
			w.walk(slot, 1, r.right_len, r.right_depth, right, right_d, r.right_end, r.right_mark, r.right_repeat);
			w.walk(slot, -1, r.left_len, r.left_depth, left, left_d, r.left_end, r.left_mark, r.left_repeat);
			w.del[slot >> 3] |= (uint8_t)(0x80u >> (slot & 7u));
			std::reverse(left.begin(), left.end());
			std::reverse(left_d.begin(), left_d.end());
			const double avg = (double)(r.left_depth + r.right_depth) / (double)(r.left_len + r.right_len);
			uint32_t md = (uint32_t)(int)avg & 0xffu;
			if (md == 10 || md == 62) --md;
			r.mid_depth = (uint8_t)md;
			const std::string kmer = w.text(slot);
			h_rec.push_back(r);
			h_bases.push_back(left + kmer + right);
			h_depths.push_back(left_d + std::string(c->p.k, (char)md) + right_d);
		}
	}
	tm.ms_host_walk = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

	// both lists ascend by the slot the scan finds the contig at: merge
	const uint64_t n_host = h_rec.size(), n_all = n_kernel + n_host;
	c->records.reserve(n_all);
	c->offsets.reserve(n_all + 1);
	for (uint64_t a = 0, b = 0; a < n_kernel || b < n_host;) {
		if (b == n_host || (a < n_kernel && k_rec[a].anchor < h_rec[b].anchor)) {
			c->records.push_back(k_rec[a]);
			c->bases.insert(c->bases.end(), k_bases.begin() + k_off[a], k_bases.begin() + k_off[a + 1]);
			c->depths.insert(c->depths.end(), k_depths.begin() + k_off[a], k_depths.begin() + k_off[a + 1]);
			++a;
		} else {
			c->records.push_back(h_rec[b]);
			c->bases.insert(c->bases.end(), h_bases[b].begin(), h_bases[b].end());
			c->depths.insert(c->depths.end(), h_depths[b].begin(), h_depths[b].end());
			++b;
		}
		c->offsets.push_back(c->bases.size());
	}
	c->summary.contigs = n_all;
	c->summary.kernel_contigs = n_kernel;
	c->summary.host_contigs = n_host;
	c->summary.bytes = c->bases.size();
	c->summary.host_nodes = host_nodes;
	c->done = true;
	if (out) *out = c->summary;
	return DBGK_OK;
}

extern "C" int dbgk_contig_summary_get(dbgk_contig *c, dbgk_contig_summary *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	if (!c->done) return DBGK_ERR_STATE;
	*out = c->summary;
	return DBGK_OK;
}

extern "C" int dbgk_contig_results(dbgk_contig *c, uint64_t *offsets, dbgk_contig_record *records, char *bases, char *depths)
{
	if (!c) return DBGK_ERR_ARG;
	if (!c->done) return DBGK_ERR_STATE;
	if (offsets) memcpy(offsets, c->offsets.data(), c->offsets.size() * 8);
	if (records && !c->records.empty()) memcpy(records, c->records.data(), c->records.size() * sizeof(dbgk_contig_record));
	if (bases && !c->bases.empty()) memcpy(bases, c->bases.data(), c->bases.size());
	if (depths && !c->depths.empty()) memcpy(depths, c->depths.data(), c->depths.size());
	return DBGK_OK;
}

extern "C" int dbgk_contig_timing_get(dbgk_contig *c, dbgk_contig_timing *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	*out = c->timing;
	return DBGK_OK;
}
