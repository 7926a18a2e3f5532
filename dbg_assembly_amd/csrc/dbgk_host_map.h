// MAP: host side of map_reads / map_pair on the GPU (include/dbgk.h, MAP section; kernels in dbgk_map.h)

struct dbgk_map : StageDev {
	dbgk_map_params p{};
	uint32_t chunk0 = 4;          // first chunk of the seed scan's ramp (dbgk_map_set_ramp; profiles/map_measure.json)
	dbgk_handle *index = nullptr; // the finalized SEEDIDX handle of the contigs
	DevBuf<uint8_t> d_ctg;        // contig text as written
	DevBuf<uint64_t> d_ctg_off;
	uint64_t n_contigs = 0;
	// identity: accept[align_len] = the largest mis_match the reference's float test lets through, -1 = none
	std::vector<int32_t> accept;
	DevBuf<int32_t> d_accept;
	// batch buffers, grown on demand
	DevBuf<uint8_t> d_seq;
	DevBuf<uint64_t> d_off;
	DevBuf<mapk::Hit> d_hits;
	DevBuf<uint32_t> d_long;
	DevBuf<mapk::MapCounters> d_ctr;
	DevBuf<unsigned long long> d_chk; // dbgk_map_reads_device: what k_map_check_batch found
	uint64_t cap_bytes = 0, cap_reads = 0;
	StageEvents<4> ev;
	dbgk_map_stats last{};
	bool have_hits = false; // d_hits holds the 2 * last.reads hits of a batch that succeeded (dbgk_map_hits_device)
};

static_assert(sizeof(dbgk_map_hit) == 32 && sizeof(mapk::Hit) == 32, "dbgk_map_hit is eight int32");
static_assert(sizeof(dbgk_map_params) == 24, "dbgk_map_params layout");

// is_prime / find_next_prime of link_scaffold/kmerSet.cpp:56-79 (the float square root and the `i < max` bound included)
static uint64_t map_find_next_prime(uint64_t num)
{
	auto is_prime = [](uint64_t n) {
		if (n < 4) return true;
		if (n % 2 == 0) return false;
		const uint64_t max = (uint64_t)sqrtf((float)n);
		for (uint64_t i = 3; i < max; i += 2)
			if (n % i == 0) return false;
		return true;
	};
	if (num % 2 == 0) num++;
	while (!is_prime(num)) num += 2;
	return num;
}

// the decision of map_reads.cpp:472 / map_pair.cpp:288 with the reference's own expression (map_func.cpp:298)
static bool map_accepts(int mis_match, int align_len, double min_identity)
{
	float identity = 1.0 - (float)mis_match / align_len;
	return !(identity < min_identity);
}

static void map_free_contigs(dbgk_map *m)
{
	if (m->index) (void)dbgk_destroy(m->index);
	m->index = nullptr;
	(void)hipSetDevice(m->device);
	m->d_ctg.release(); m->d_ctg_off.release();
	m->n_contigs = 0;
}

extern "C" int dbgk_map_create(const dbgk_map_params *p, int device, dbgk_map **out)
{
	if (!p || !out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (p->k < 1 || p->k > 31 || p->seed_kmers < 1 || p->seed_kmers > (1 << 29) || p->min_read_len < 0 ||
	    (p->second_alignment != 0 && p->second_alignment != 1) || p->min_identity != p->min_identity || device < 0)
		return DBGK_ERR_ARG;
	dbgk_map *m = new (std::nothrow) dbgk_map;
	if (!m) return DBGK_ERR_NOMEM;
	m->p = *p;
	int rc = stage_open(*m, device);
	if (!rc) rc = m->ev.create();
	if (!rc) rc = m->d_ctr.reserve(sizeof(mapk::MapCounters));
	if (rc) {
		dbgk_map_destroy(m);
		return rc;
	}
	*out = m;
	return DBGK_OK;
}

extern "C" int dbgk_map_destroy(dbgk_map *m)
{
	if (!m) return DBGK_ERR_ARG;
	stage_drain(m->device, m->stream);
	if (m->index) (void)dbgk_destroy(m->index);
	delete m;
	return DBGK_OK;
}

extern "C" int dbgk_map_set_ramp(dbgk_map *m, uint32_t first_chunk)
{
	if (!m || first_chunk < 1 || first_chunk > 64) return DBGK_ERR_ARG;
	m->chunk0 = first_chunk;
	return DBGK_OK;
}

extern "C" int dbgk_map_set_contigs(dbgk_map *m, const char *bases, const uint64_t *offsets, uint64_t n_contigs)
{
	if (!m || !offsets || offsets[0] != 0 || n_contigs >= (1ull << 31)) return DBGK_ERR_ARG;
	uint64_t longest = 0;
	for (uint64_t i = 0; i < n_contigs; ++i) {
		if (offsets[i + 1] < offsets[i]) return DBGK_ERR_ARG;
		longest = std::max<uint64_t>(longest, offsets[i + 1] - offsets[i]);
	}
	const uint64_t total = offsets[n_contigs];
	if ((total && !bases) || longest >= (1ull << 30)) return DBGK_ERR_ARG; // pos is a 30-bit field of the index
	map_free_contigs(m);
	m->have_hits = false;
	// the index: init_kmerset(total * 3) of map_pair.cpp:122-124 -- find_next_prime unless below 3
	dbgk_config cfg{};
	cfg.kmer_size = m->p.k;
	cfg.max_read_len = 0x7FFFFFFF;
	cfg.table_slots = total * 3 < 3 ? 3 : map_find_next_prime(total * 3);
	cfg.device_id = m->device;
	cfg.engine = DBGK_ENGINE_SEEDIDX;
	cfg.max_batch_bases = std::max<uint64_t>(std::max<uint64_t>(std::min<uint64_t>(total, 256ull << 20), longest) + 64, 1ull << 20);
	int rc = dbgk_create(&cfg, &m->index);
	if (rc) return rc;
	if (n_contigs) rc = dbgk_push_reads(m->index, bases, offsets, n_contigs);
	dbgk_stats st;
	if (!rc) rc = dbgk_finalize(m->index, &st);
	if (rc) {
		map_free_contigs(m);
		return rc;
	}
	HIPCHK(hipSetDevice(m->device));
	if (m->d_ctg.reserve(total + 16) || m->d_ctg_off.reserve((n_contigs + 1) * 8)) {
		map_free_contigs(m);
		return DBGK_ERR_NOMEM;
	}
	if (total) HIPCHK(hipMemcpyAsync(m->d_ctg, bases, total, hipMemcpyHostToDevice, m->stream));
	HIPCHK(hipMemcpyAsync(m->d_ctg_off, offsets, (n_contigs + 1) * 8, hipMemcpyHostToDevice, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	m->n_contigs = n_contigs;
	return DBGK_OK;
}

// accept[] through align_len = max_len, on the device
static int map_ensure_accept(dbgk_map *m, uint64_t max_len)
{
	if (m->accept.size() > max_len) return DBGK_OK;
	const uint64_t from = m->accept.size();
	m->accept.resize(max_len + 1);
	for (uint64_t len = from; len <= max_len; ++len) {
		// the test is monotone in mis_match: bisect for the last accepted count
		int64_t lo = -1, hi = (int64_t)len; // lo: accepted (or none), hi: upper end of the candidates
		while (lo < hi) {
			const int64_t mid = lo + (hi - lo + 1) / 2;
			if (len && map_accepts((int)mid, (int)len, m->p.min_identity)) lo = mid; else hi = mid - 1;
		}
		m->accept[len] = (int32_t)lo;
	}
	if (m->d_accept.reserve(m->accept.size() * 4, 4096 * 4)) return DBGK_ERR_NOMEM;
	HIPCHK(hipMemcpyAsync(m->d_accept, m->accept.data(), m->accept.size() * 4, hipMemcpyHostToDevice, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	return DBGK_OK;
}

// batch buffers for n_reads reads and, for a batch that is uploaded, n_bytes bytes of them
static int map_ensure_batch(dbgk_map *m, uint64_t n_bytes, uint64_t n_reads)
{
	if (n_bytes + 16 > m->cap_bytes || n_reads > m->cap_reads) {
		const uint64_t bytes = std::max<uint64_t>(n_bytes + 16, 1 << 20), reads = std::max<uint64_t>(n_reads, 1 << 14);
		m->cap_bytes = m->cap_reads = 0;
		if (m->d_seq.reserve(bytes) || m->d_off.reserve((reads + 1) * 8) || m->d_hits.reserve(reads * 2 * sizeof(mapk::Hit)) || m->d_long.reserve(reads * 4))
			return DBGK_ERR_NOMEM;
		m->cap_bytes = bytes;
		m->cap_reads = reads;
	}
	return DBGK_OK;
}

// The n_reads > 0 reads of d_seq / d_off (on the device, or on their way there on the mapper's stream) -> out, or with a null `out`
// left in d_hits alone.  The accept table covers the longest read and the batch buffers hold n_reads reads.
static int map_run(dbgk_map *m, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_reads, dbgk_map_hit *out)
{
	HIPCHK(hipMemsetAsync(m->d_ctr, 0, sizeof(mapk::MapCounters), m->stream));
	const mapk::MapParams P{m->p.k, m->p.seed_kmers, m->p.min_read_len, m->p.second_alignment, m->chunk0, (uint32_t)m->accept.size()};
	const mapk::MapIndex X{m->index->tref(), m->index->h_ctr->polyA_links, m->d_ctg, m->d_ctg_off, (uint32_t)m->n_contigs};
	const uint32_t nr = (uint32_t)n_reads;
	const uint64_t groups = (n_reads + mapk::kMapWaves - 1) / mapk::kMapWaves;
	const unsigned grid = (unsigned)std::min<uint64_t>(groups, (uint64_t)m->n_cu * 32);
	HIPCHK(hipEventRecord(m->ev[0], m->stream));
	hipLaunchKernelGGL(mapk::k_map_reads<false>, dim3(grid), dim3(mapk::kMapWaves * 64), 0, m->stream, d_seq, d_off, nr, P, X,
	                   (const int32_t *)m->d_accept.p, m->d_hits, m->d_long, m->d_ctr);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(m->ev[1], m->stream));
	mapk::MapCounters hc{};
	HIPCHK(hipMemcpyAsync(&hc, m->d_ctr, sizeof hc, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	if (hc.n_long) { // reads beyond the LDS slice: the same code out of global memory
		const unsigned grid_long = (unsigned)std::min<uint64_t>((hc.n_long + mapk::kMapWaves - 1) / mapk::kMapWaves, (uint64_t)m->n_cu * 32);
		HIPCHK(hipEventRecord(m->ev[2], m->stream));
		hipLaunchKernelGGL(mapk::k_map_reads<true>, dim3(grid_long), dim3(mapk::kMapWaves * 64), 0, m->stream, d_seq, d_off, nr, P, X,
		                   (const int32_t *)m->d_accept.p, m->d_hits, m->d_long, m->d_ctr);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(m->ev[3], m->stream));
		HIPCHK(hipMemcpyAsync(&hc, m->d_ctr, sizeof hc, hipMemcpyDeviceToHost, m->stream));
	}
	if (out) HIPCHK(hipMemcpyAsync(out, m->d_hits, n_reads * 2 * sizeof(mapk::Hit), hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	m->have_hits = true;
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
	m->last.ms_map = ms;
	if (hc.n_long) {
		HIPCHK(hipEventElapsedTime(&ms, m->ev[2], m->ev[3]));
		m->last.ms_long = ms;
	}
	m->last.by_lds = hc.by_lds;
	m->last.by_long = hc.by_long;
	m->last.skipped = hc.skipped;
	m->last.windows_probed = hc.windows;
	return DBGK_OK;
}

extern "C" int dbgk_map_reads(dbgk_map *m, const char *bases, const uint64_t *offsets, uint64_t n_reads, dbgk_map_hit *out)
{
	if (!m || !offsets || (n_reads && !out)) return DBGK_ERR_ARG;
	if (offsets[0] != 0 || n_reads >= (1ull << 31)) return DBGK_ERR_ARG;
	uint64_t max_len = 0;
	for (uint64_t i = 0; i < n_reads; ++i) {
		if (offsets[i + 1] < offsets[i]) return DBGK_ERR_ARG;
		max_len = std::max<uint64_t>(max_len, offsets[i + 1] - offsets[i]);
	}
	if (max_len >= (1ull << 31) || (n_reads && offsets[n_reads] && !bases)) return DBGK_ERR_ARG;
	if (!m->index) return DBGK_ERR_STATE;
	m->last = dbgk_map_stats{};
	m->last.reads = n_reads;
	m->have_hits = !n_reads;
	if (!n_reads) return DBGK_OK;
	HIPCHK(hipSetDevice(m->device));
	int rc = map_ensure_accept(m, max_len);
	if (rc) return rc;
	// stage the batch
	const uint64_t nb = offsets[n_reads];
	rc = map_ensure_batch(m, nb, n_reads);
	if (rc) return rc;
	if (nb) HIPCHK(hipMemcpyAsync(m->d_seq, bases, nb, hipMemcpyHostToDevice, m->stream));
	HIPCHK(hipMemcpyAsync(m->d_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, m->stream));
	return map_run(m, m->d_seq, m->d_off, n_reads, out);
}

// both device entries; keep: the hits stay on the device and `out` is not looked at
static int map_reads_device(dbgk_map *m, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t max_len, dbgk_map_hit *out,
                            bool keep)
{
	if (!m || (n_reads && ((!keep && !out) || !d_offsets)) || n_reads >= (1ull << 31) || max_len >= (1ull << 31)) return DBGK_ERR_ARG;
	if (((uintptr_t)d_bases & 15u) || ((uintptr_t)d_offsets & 7u) || (n_bases && !d_bases)) return DBGK_ERR_ARG;
	if (!m->index) return DBGK_ERR_STATE;
	m->last = dbgk_map_stats{};
	m->last.reads = n_reads;
	m->have_hits = !n_reads;
	if (!n_reads) return DBGK_OK;
	HIPCHK(hipSetDevice(m->device));
	// what dbgk_map_reads learns from its host loop over the offsets, learned on the device, before any read is mapped
	if (m->d_chk.reserve(3 * sizeof(unsigned long long))) return DBGK_ERR_NOMEM;
	unsigned long long chk[3] = {0, 0, 0};
	HIPCHK(hipMemsetAsync(m->d_chk, 0, sizeof chk, m->stream));
	hipLaunchKernelGGL(mapk::k_map_check_batch, dim3((unsigned)std::min<uint64_t>((n_reads + 255) / 256, (uint64_t)m->n_cu * 16)), dim3(256), 0,
	                   m->stream, d_offsets, (uint32_t)n_reads, m->d_chk);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(chk, m->d_chk, sizeof chk, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	if (chk[1] || chk[0] > max_len || chk[2] > n_bases) return DBGK_ERR_ARG;
	int rc = map_ensure_accept(m, max_len);
	if (rc) return rc;
	rc = map_ensure_batch(m, 0, n_reads);
	if (rc) return rc;
	return map_run(m, (const uint8_t *)d_bases, d_offsets, n_reads, keep ? nullptr : out);
}

extern "C" int dbgk_map_reads_device(dbgk_map *m, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t max_len,
                                     dbgk_map_hit *out)
{
	return map_reads_device(m, d_bases, d_offsets, n_reads, n_bases, max_len, out, false);
}

extern "C" int dbgk_map_reads_device_keep(dbgk_map *m, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t max_len)
{
	return map_reads_device(m, d_bases, d_offsets, n_reads, n_bases, max_len, nullptr, true);
}

extern "C" int dbgk_map_hits_device(dbgk_map *m, const dbgk_map_hit **d_hits, uint64_t *n_reads)
{
	if (!m || !d_hits || !n_reads) return DBGK_ERR_ARG;
	if (!m->have_hits) return DBGK_ERR_STATE;
	*d_hits = m->last.reads ? reinterpret_cast<const dbgk_map_hit *>(m->d_hits.p) : nullptr;
	*n_reads = m->last.reads;
	return DBGK_OK;
}

extern "C" int dbgk_map_batch_stats(dbgk_map *m, dbgk_map_stats *out)
{
	if (!m || !out) return DBGK_ERR_ARG;
	*out = m->last;
	return DBGK_OK;
}
