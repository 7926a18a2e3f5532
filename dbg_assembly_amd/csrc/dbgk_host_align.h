// ALIGN: host side of the batched global alignments (include/dbgk.h, SIMPLIFY section; kernel in dbgk_align.h).  Works on a CONTIG
// handle (dbgk_host_contig.h) and uses its device, stream and events only: an alignment depends on its two strings, not on a table.
//
// A call goes through its pairs in batches.  Per batch the sequences of the pairs that fit DBGK_ALIGN_MAX_LEN go up back to back, the
// kernel aligns one pair per wave, and rows and aligned strings come back; a pair's strings have len_i + len_j bytes of room on the
// device (an alignment has no more columns) and are packed to their columns here.  A batch is as many pairs as keep sequences and
// strings within kAlignBudget bytes (at most kAlignMaxPairs); the test hook align_batch=N makes it N pairs.  A pair above the bound
// never reaches the device.

namespace {

constexpr uint64_t kAlignBudget = 64ull << 20;
constexpr uint64_t kAlignMaxPairs = 1ull << 20;

static_assert(sizeof(dbgk_align_row) == 24 && sizeof(alignk::Row) == 24 && offsetof(dbgk_align_row, score) == 8 && offsetof(alignk::Row, score) == 8 &&
              offsetof(dbgk_align_row, status) == 20 && offsetof(alignk::Row, status) == 20, "dbgk_align_row layout");
static_assert(sizeof(dbgk_align_summary) == 48 && sizeof(dbgk_align_timing) == 56 && offsetof(dbgk_align_timing, ms_align) == 48, "ALIGN layouts");
static_assert(DBGK_ALIGN_MAX_LEN == alignk::kAlignMaxLen && DBGK_ALIGN_MAX_LEN >= 256, "the kernel's bound is the header's");

// pairs [p0, p1) of the call: those that fit the bound through the kernel, results into the handle
int align_batch(dbgk_contig *c, const char *seqs, const uint64_t *offsets, uint64_t p0, uint64_t p1)
{
	using namespace alignk;
	std::vector<uint64_t> which, off(1, 0), out_off(1, 0);
	std::vector<uint8_t> bytes;
	uint64_t cells = 0;
	for (uint64_t p = p0; p < p1; ++p) {
		if (c->align_rows[p].status != DBGK_ALIGN_DONE) continue;
		which.push_back(p);
		for (int s = 0; s < 2; ++s) {
			bytes.insert(bytes.end(), seqs + offsets[2 * p + s], seqs + offsets[2 * p + s + 1]);
			off.push_back(bytes.size());
		}
		out_off.push_back(bytes.size());
		cells += (uint64_t)c->align_rows[p].len_i * c->align_rows[p].len_j;
	}
	const uint64_t m = which.size(), room = bytes.size();
	if (!m) return DBGK_OK;
	ContigScratch mem;
	uint8_t *d_seqs = nullptr, *d_out_i = nullptr, *d_out_j = nullptr;
	uint64_t *d_off = nullptr, *d_out_off = nullptr;
	Row *d_rows = nullptr;
	if (!mem.get(d_seqs, room) || !mem.get(d_off, 2 * m + 1) || !mem.get(d_out_off, m + 1) || !mem.get(d_rows, m) || !mem.get(d_out_i, room) ||
	    !mem.get(d_out_j, room))
		return DBGK_ERR_NOMEM;
	HIPCHK(hipMemcpyAsync(d_seqs, bytes.data(), room, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_off, off.data(), (2 * m + 1) * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_out_off, out_off.data(), (m + 1) * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipEventRecord(c->ev[0], c->stream));
	const unsigned grid = (unsigned)std::min<uint64_t>(m, (uint64_t)c->n_cu * 8);   // eight workgroups' LDS fit a CU
	hipLaunchKernelGGL(k_align_pairs, dim3(grid), dim3(kAlignThreads), 0, c->stream, d_seqs, d_off, (uint32_t)m, d_out_off, d_rows, d_out_i, d_out_j);
	dbgk_align_timing &tm = c->align_timing;
	const int rc = simplify_elapsed(c, tm.ms_align);
	if (rc) return rc;
	std::vector<dbgk_align_row> rows(m);
	std::vector<char> out_i(room), out_j(room);
	HIPCHK(hipMemcpy(rows.data(), d_rows, m * sizeof(Row), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out_i.data(), d_out_i, room, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out_j.data(), d_out_j, room, hipMemcpyDeviceToHost));
	for (uint64_t x = 0; x < m; ++x) {
		const dbgk_align_row &r = rows[x];
		const dbgk_align_row &want = c->align_rows[which[x]];
		if (r.status != DBGK_ALIGN_DONE || r.len_i != want.len_i || r.len_j != want.len_j || r.aligned_len > (uint64_t)r.len_i + r.len_j) {
			g_last_error = "the alignment kernel returned a row that does not belong to its pair";
			return DBGK_ERR_HIP;
		}
	}
	// the strings stay per pair until the call has all of them: align_first is filled at its end
	for (uint64_t x = 0; x < m; ++x) {
		c->align_rows[which[x]] = rows[x];
		c->align_i.insert(c->align_i.end(), out_i.begin() + out_off[x], out_i.begin() + out_off[x] + rows[x].aligned_len);
		c->align_j.insert(c->align_j.end(), out_j.begin() + out_off[x], out_j.begin() + out_off[x] + rows[x].aligned_len);
	}
	tm.bytes_up += room + (3 * m + 2) * 8;
	tm.bytes_back += m * sizeof(Row) + 2 * room;
	tm.pairs += m;
	tm.cells += cells;
	++tm.batches;
	++c->align_summary.batches;
	return DBGK_OK;
}

} // namespace

extern "C" int dbgk_align_pairs(dbgk_contig *c, const char *seqs, const uint64_t *offsets, uint64_t n_pairs, dbgk_align_summary *out)
{
	if (!c || (n_pairs && (!seqs || !offsets))) return DBGK_ERR_ARG;
	for (uint64_t s = 0; s < 2 * n_pairs; ++s) {
		if (offsets[s + 1] <= offsets[s]) return DBGK_ERR_ARG;   // decreasing, or a sequence of length 0
		for (uint64_t x = offsets[s]; x < offsets[s + 1]; ++x)
			if (seqs[x] != 'A' && seqs[x] != 'C' && seqs[x] != 'G' && seqs[x] != 'T') return DBGK_ERR_ARG;
	}
	c->aligned = false;
	c->align_rows.assign(n_pairs, dbgk_align_row{});
	c->align_first.assign(n_pairs + 1, 0);
	c->align_i.clear();
	c->align_j.clear();
	c->align_summary = dbgk_align_summary{};
	c->align_summary.pairs = n_pairs;
	for (uint64_t p = 0; p < n_pairs; ++p) {
		dbgk_align_row &r = c->align_rows[p];
		const uint64_t li = offsets[2 * p + 1] - offsets[2 * p], lj = offsets[2 * p + 2] - offsets[2 * p + 1];
		const bool fits = li <= DBGK_ALIGN_MAX_LEN && lj <= DBGK_ALIGN_MAX_LEN;
		r.len_i = (uint32_t)std::min<uint64_t>(li, 0xffffffffull);
		r.len_j = (uint32_t)std::min<uint64_t>(lj, 0xffffffffull);
		r.status = fits ? DBGK_ALIGN_DONE : DBGK_ALIGN_TOO_LONG;
		(fits ? c->align_summary.aligned : c->align_summary.too_long)++;
	}
	if (c->align_summary.aligned) {
		HIPCHK(hipSetDevice(c->device));
		const char *hook = dbgk_hook("align_batch");
		const uint64_t hook_pairs = hook ? std::max<uint64_t>(1, std::min<uint64_t>(strtoull(hook, nullptr, 10), kAlignMaxPairs)) : 0;
		for (uint64_t p0 = 0; p0 < n_pairs;) {
			uint64_t p1 = p0, room = 0;
			while (p1 < n_pairs && p1 - p0 < (hook_pairs ? hook_pairs : kAlignMaxPairs)) {
				const uint64_t add = c->align_rows[p1].status == DBGK_ALIGN_DONE ? 3 * (uint64_t)(c->align_rows[p1].len_i + c->align_rows[p1].len_j) : 0;
				if (!hook_pairs && p1 > p0 && room + add > kAlignBudget) break;
				room += add;
				++p1;
			}
			const int rc = align_batch(c, seqs, offsets, p0, p1);
			if (rc) return rc;
			p0 = p1;
		}
	}
	for (uint64_t p = 0; p < n_pairs; ++p) c->align_first[p + 1] = c->align_first[p] + c->align_rows[p].aligned_len;
	c->align_summary.aligned_bytes = c->align_first[n_pairs];
	c->aligned = true;
	if (out) *out = c->align_summary;
	return DBGK_OK;
}

extern "C" int dbgk_align_results(dbgk_contig *c, dbgk_align_row *rows, uint64_t *aligned_offsets, char *aligned_i, char *aligned_j)
{
	if (!c) return DBGK_ERR_ARG;
	if (!c->aligned) return DBGK_ERR_STATE;
	if (rows && !c->align_rows.empty()) memcpy(rows, c->align_rows.data(), c->align_rows.size() * sizeof(dbgk_align_row));
	if (aligned_offsets) memcpy(aligned_offsets, c->align_first.data(), c->align_first.size() * 8);
	if (aligned_i && !c->align_i.empty()) memcpy(aligned_i, c->align_i.data(), c->align_i.size());
	if (aligned_j && !c->align_j.empty()) memcpy(aligned_j, c->align_j.data(), c->align_j.size());
	return DBGK_OK;
}

extern "C" int dbgk_align_timing_get(dbgk_contig *c, dbgk_align_timing *out)
{
	if (!c || !out) return DBGK_ERR_ARG;
	*out = c->align_timing;
	return DBGK_OK;
}
