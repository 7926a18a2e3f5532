// dbgk_host_wide_links.h -- the WIDE host table together with the consumer's first pass (calculate_kmer_links, contig.cpp:107-181):
// dbgk_export_host_table_links for 32-byte nodes.  k_wide_kmer_links reads the device table in place; the nodes the host puts on
// their chains afterwards (zero low word, key 0) are patched in by dbgk_wide_links_patch.h.  PARITY UNPINNED above k = 32.

// the link pass of one handle over its own slots (a shard: its slot range): device buffers, block counts, results of PASS 0
struct WideLinkPass {
	dbgk_handle *h;
	uint64_t n_blocks;
	DevBuf<uint16_t> d_klink;
	DevBuf<uint8_t> d_del;
	DevBuf<unsigned long long> d_stats, d_base, d_tips, d_branches;
	DevBuf<uint32_t> d_counts;
	std::vector<unsigned long long> base;
	unsigned long long res[261];
	uint64_t nt = 0, nb = 0;
	const bool timing;                // DBGK_TIMINGS, read once per export
	float kernel_ms[2] = {0.f, 0.f}; // ... the device time of the two launches
	StageEvent ev[2];

	// around the launch of one PASS: the two events when its device time is wanted
	int before_launch()
	{
		if (!timing) return DBGK_OK;
		if (ev[0].create() || ev[1].create()) return DBGK_ERR_HIP;
		HIPCHK(hipEventRecord(ev[0], h->stream));
		return DBGK_OK;
	}
	int after_launch(int pass)
	{
		HIPCHK(hipGetLastError());
		if (!timing) return DBGK_OK;
		HIPCHK(hipEventRecord(ev[1], h->stream));
		HIPCHK(hipEventSynchronize(ev[1]));
		HIPCHK(hipEventElapsedTime(&kernel_ms[pass], ev[0], ev[1]));
		return DBGK_OK;
	}

	WideLinkPass(dbgk_handle *handle, bool want_timing) : h(handle), n_blocks((handle->tslots + kLinkChunk - 1) / kLinkChunk), timing(want_timing) {}
	WideLinkPass(const WideLinkPass &) = delete;
	WideLinkPass &operator=(const WideLinkPass &) = delete;
	~WideLinkPass() { (void)hipSetDevice(h->device); } // (the buffers and events go after this body has run)

	// PASS 0: klink[tslots] and del_flag[tslots / 8 + 1] of the handle's slots, res, nt / nb
	int count(int32_t cutoff, uint16_t *klink, uint8_t *del_flag)
	{
		const uint64_t size = h->tslots;
		int rc = use_device(h);
		if (rc) return rc;
		if (d_klink.reserve(size * 2) || d_del.reserve(size / 8 + 1) || d_stats.reserve(261 * 8) || d_counts.reserve(n_blocks * 8) || d_base.reserve(n_blocks * 16))
			return DBGK_ERR_NOMEM;
		HIPCHK(hipMemsetAsync(d_stats, 0, 261 * 8, h->stream));
		HIPCHK(hipMemsetAsync(d_del, 0, size / 8 + 1, h->stream));
		if ((rc = before_launch())) return rc;
		hipLaunchKernelGGL(k_wide_kmer_links<0>, dim3((unsigned)n_blocks), dim3(kBlock), 0, h->stream, h->wnodes, size, (int)cutoff, (uint64_t)0, d_klink, d_del,
		                   d_stats, d_counts, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr);
		if ((rc = after_launch(0))) return rc;
		std::vector<uint32_t> counts(n_blocks * 2);
		HIPCHK(hipMemcpyAsync(counts.data(), d_counts, n_blocks * 8, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipMemcpyAsync(res, d_stats, sizeof res, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipMemcpyAsync(klink, d_klink, size * 2, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipMemcpyAsync(del_flag, d_del, size / 8 + 1, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
		base.resize(n_blocks * 2);
		for (uint64_t b = 0; b < n_blocks; b++) {
			base[2 * b] = nt;
			base[2 * b + 1] = nb;
			nt += counts[2 * b];
			nb += counts[2 * b + 1];
		}
		return DBGK_OK;
	}

	// PASS 1: the nt tip and nb branch slots, ascending, as slot_base + slot; either list may be null
	int lists(int32_t cutoff, uint64_t slot_base, uint64_t *tips, uint64_t *branches)
	{
		if ((!tips && !branches) || (!nt && !nb)) return DBGK_OK;
		int rc = use_device(h);
		if (rc) return rc;
		if (d_tips.reserve((nt ? nt : 1) * 8) || d_branches.reserve((nb ? nb : 1) * 8)) return DBGK_ERR_NOMEM;
		HIPCHK(hipMemcpyAsync(d_base, base.data(), n_blocks * 16, hipMemcpyHostToDevice, h->stream));
		if ((rc = before_launch())) return rc;
		hipLaunchKernelGGL(k_wide_kmer_links<1>, dim3((unsigned)n_blocks), dim3(kBlock), 0, h->stream, h->wnodes, h->tslots, (int)cutoff, slot_base, d_klink, d_del,
		                   d_stats, d_counts, d_base, d_tips, d_branches);
		if ((rc = after_launch(1))) return rc;
		if (tips && nt) HIPCHK(hipMemcpyAsync(tips, d_tips, nt * 8, hipMemcpyDeviceToHost, h->stream));
		if (branches && nb) HIPCHK(hipMemcpyAsync(branches, d_branches, nb * 8, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
		return DBGK_OK;
	}

	void add_stats(dbgk_link_stats *st) const
	{
		for (int i = 0; i < 256; i++) st->depth_stat[i] += (int64_t)res[i];
		st->total_nodes += (int64_t)res[256];
		st->deleted_lowfreq += (int64_t)res[257];
		st->linear_nodes += (int64_t)res[258];
		st->tip_nodes += (int64_t)res[259];
		st->branch_nodes += (int64_t)res[260];
	}
};

// after PASS 0 of every part (parts in ascending slot-range order): the lists if they fit, then the placed nodes
static int wide_links_finish(std::vector<WideLinkPass *> &parts, const std::vector<uint64_t> &slot_lo, const std::vector<PlacedNode> &placed, const LinkOutputs &LO)
{
	uint64_t nt = 0, nb = 0;
	for (const WideLinkPass *p : parts) {
		nt += p->nt;
		nb += p->nb;
	}
	const bool fits = (!LO.tips || nt <= LO.tip_cap) && (!LO.branches || nb <= LO.branch_cap);
	if (fits) {
		uint64_t at = 0, ab = 0;
		for (size_t i = 0; i < parts.size(); i++) {
			int rc = parts[i]->lists(LO.cutoff, slot_lo[i], LO.tips ? LO.tips + at : nullptr, LO.branches ? LO.branches + ab : nullptr);
			if (rc) return rc;
			at += parts[i]->nt;
			ab += parts[i]->nb;
		}
	}
	if (LO.stats) {
		memset(LO.stats, 0, sizeof *LO.stats);
		for (const WideLinkPass *p : parts) p->add_stats(LO.stats);
	}
	*LO.n_tips = nt;
	*LO.n_branches = nb;
	if (parts[0]->timing) {
		float ms[2] = {0.f, 0.f};
		for (const WideLinkPass *p : parts) ms[0] += p->kernel_ms[0], ms[1] += p->kernel_ms[1];
		fprintf(stderr, "dbgk wide link pass, device (ms): records, flags and counts %.3f, lists %.3f (%zu handle%s, %zu nodes placed on the host)\n", ms[0], ms[1],
		        parts.size(), parts.size() == 1 ? "" : "s", placed.size());
	}
	// (lists that do not fit even without the placed nodes: counts only, the lists stay untouched)
	const int rc = patch_placed_links(placed, LO.cutoff, LO.klink, LO.del_flag, fits ? LO.tips : nullptr, LO.tip_cap, LO.n_tips, fits ? LO.branches : nullptr,
	                                  LO.branch_cap, LO.n_branches, LO.stats);
	return fits ? rc : DBGK_ERR_CAPACITY;
}

static LinkOutputs wide_link_outputs(int32_t cutoff, uint16_t *klink, uint8_t *del_flag, uint64_t *tip_nodes, uint64_t tip_capacity, uint64_t *n_tips,
                                     uint64_t *branch_nodes, uint64_t branch_capacity, uint64_t *n_branches, dbgk_link_stats *stats)
{
	LinkOutputs LO;
	LO.cutoff = cutoff;
	LO.klink = klink;
	LO.del_flag = del_flag;
	LO.tips = tip_nodes;
	LO.branches = branch_nodes;
	LO.tip_cap = tip_nodes ? tip_capacity : 0;
	LO.branch_cap = branch_nodes ? branch_capacity : 0;
	LO.n_tips = n_tips;
	LO.n_branches = n_branches;
	LO.stats = stats;
	return LO;
}

extern "C" int dbgk_wide_export_host_table_links(dbgk_handle *h, uint64_t host_size, dbgk_node32 *array, uint8_t *nul_flag, int32_t kmer_freq_cutoff,
                                                 uint16_t *klink, uint8_t *del_flag, uint64_t *tip_nodes, uint64_t tip_capacity, uint64_t *n_tips,
                                                 uint64_t *branch_nodes, uint64_t branch_capacity, uint64_t *n_branches, dbgk_link_stats *stats)
{
	if (!h || !array || !nul_flag || !klink || !del_flag || !n_tips || !n_branches) return DBGK_ERR_ARG;
	if (!h->wide || h->sharded) return DBGK_ERR_STATE; // slot numbers are those of ONE table: shards go through dbgk_comm_wide_export_host_table_links
	std::vector<PlacedNode> placed;
	int rc = wide_export_host_table_impl(h, host_size, array, nul_flag, &placed);
	if (rc) return rc;
	WideLinkPass P(h, getenv("DBGK_TIMINGS") != nullptr);
	rc = P.count(kmer_freq_cutoff, klink, del_flag);
	if (rc) return rc;
	std::vector<WideLinkPass *> parts{&P};
	return wide_links_finish(parts, {0}, placed,
	                         wide_link_outputs(kmer_freq_cutoff, klink, del_flag, tip_nodes, tip_capacity, n_tips, branch_nodes, branch_capacity, n_branches, stats));
}

// several shards of one table: the pass per shard on its slot range, slices and lists put side by side in ascending slot-range
// order, then the nodes placed over the WHOLE table
extern "C" int dbgk_comm_wide_export_host_table_links(dbgk_comm *c, uint64_t host_size, dbgk_node32 *array, uint8_t *nul_flag, int32_t kmer_freq_cutoff,
                                                      uint16_t *klink, uint8_t *del_flag, uint64_t *tip_nodes, uint64_t tip_capacity, uint64_t *n_tips,
                                                      uint64_t *branch_nodes, uint64_t branch_capacity, uint64_t *n_branches, dbgk_link_stats *stats)
{
	if (!c || !array || !nul_flag || !klink || !del_flag || !n_tips || !n_branches) return DBGK_ERR_ARG;
	if (!c->finalized || !c->wide) return DBGK_ERR_STATE;
	std::vector<dbgk_handle *> order(c->h.begin(), c->h.end());
	std::sort(order.begin(), order.end(), [](const dbgk_handle *a, const dbgk_handle *b) { return a->wgeom.slot_lo < b->wgeom.slot_lo; });
	uint64_t end = 0;
	bool tiled = true;
	for (const dbgk_handle *h : order) { // the ranges tile [0, host_size) without overlap, each starting on a del_flag byte
		tiled = tiled && h->wgeom.slot_lo == end && !(h->wgeom.slot_lo & 7u);
		end += h->tslots;
	}
	if (!tiled || end != host_size) { // (before anything is written)
		g_last_error = "dbgk_comm_wide_export_host_table_links: the shards' slot ranges do not tile a table of host_size slots";
		return host_size != c->h[0]->size ? DBGK_ERR_ARG : DBGK_ERR_STATE;
	}
	std::vector<PlacedNode> placed;
	int rc = comm_wide_export_host_table_impl(c, host_size, array, nul_flag, &placed);
	if (rc) return rc;
	const bool timing = getenv("DBGK_TIMINGS") != nullptr;
	memset(del_flag, 0, host_size / 8 + 1);
	std::vector<std::unique_ptr<WideLinkPass>> own;
	std::vector<WideLinkPass *> parts;
	std::vector<uint64_t> slot_lo;
	std::vector<uint8_t> del;
	for (dbgk_handle *h : order) {
		own.emplace_back(new WideLinkPass(h, timing));
		parts.push_back(own.back().get());
		slot_lo.push_back(h->wgeom.slot_lo);
		del.assign(h->tslots / 8 + 1, 0);
		rc = parts.back()->count(kmer_freq_cutoff, klink + h->wgeom.slot_lo, del.data());
		if (rc) return rc;
		memcpy(del_flag + h->wgeom.slot_lo / 8, del.data(), (h->tslots + 7) / 8);
	}
	return wide_links_finish(parts, slot_lo, placed,
	                         wide_link_outputs(kmer_freq_cutoff, klink, del_flag, tip_nodes, tip_capacity, n_tips, branch_nodes, branch_capacity, n_branches, stats));
}
