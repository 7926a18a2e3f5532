// INFLATE stage, host side (include/dbgk.h, INFLATE section; kernels in dbgk_inflate.h, the decode core in dbgk_inflate_core.h).  One
// call: the member table goes up, k_inf_sizes and the scan of ISIZE give every member its place, one read-back of the total sizes the
// output, then decode and resolve once per round of kInfRound members.  Calls are stateless: nothing but the buffers outlives one.

struct dbgk_inf : StageDev {
	uint64_t max_out = 0;
	DevBuf<uint8_t> gz; // dbgk_inf_inflate: the uploaded members
	DevBuf<uint64_t> off, place; // cap_members + 1 each
	DevBuf<uint32_t> isize, crc, status;
	uint64_t cap_members = 0;
	DevBuf<uint32_t> tokens, n_tok; // cap_round slots of kGzPiece tokens
	uint64_t cap_round = 0;
	DevBuf<uint8_t> out;
	ScanTmp tmp; // the scan's
	DevBuf<uint32_t> x8;
	DevBuf<unsigned long long> ctr;
	StageEvents<3> ev;
	bool have = false;
	dbgk_inf_info info{};
	dbgk_inf_timing timing{};
	std::vector<uint8_t> reasons;
};

static_assert(DBGK_INF_ROUND == infk::kInfRound && DBGK_INF_FRAME == inf::R_FRAME && DBGK_INF_CRC == inf::R_CRC && DBGK_INF_FRAME + 1 == inf::R_COUNT,
              "the header's figures are the kernels'");

extern "C" int dbgk_inf_destroy(dbgk_inf *z)
{
	if (!z) return DBGK_ERR_ARG;
	stage_drain(z->device, z->stream);
	delete z;
	return DBGK_OK;
}

// the resolve kernel's LDS is above 64 KiB
static int inf_raise_lds()
{
	DBGK_LDS_ATTR(infk::k_inf_resolve, sizeof(infk::InfResolveLds));
	return DBGK_OK;
}

extern "C" int dbgk_inf_create(uint64_t max_out_bytes, dbgk_inf **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	const uint64_t top = (1ull << 31) - 65536;
	if (max_out_bytes > top) return DBGK_ERR_ARG;
	dbgk_inf *z = new (std::nothrow) dbgk_inf;
	if (!z) return DBGK_ERR_NOMEM;
	z->max_out = max_out_bytes ? max_out_bytes : top;
	int rc = stage_open(*z, kStageCurrentDevice);
	if (!rc) rc = z->ev.create();
	if (!rc && (z->x8.reserve(16 * 4) || z->ctr.reserve(infk::IC_COUNT * 8))) rc = DBGK_ERR_NOMEM;
	if (!rc) {
		const gzf::GzPowers t = gzf::gz_powers();
		if (hipMemcpy(z->x8, t.x8, 16 * 4, hipMemcpyHostToDevice) != hipSuccess) rc = DBGK_ERR_HIP;
	}
	if (!rc) rc = inf_raise_lds();
	if (rc) {
		dbgk_inf_destroy(z);
		return rc;
	}
	*out = z;
	return DBGK_OK;
}

// (the stream is idle)
static int inf_ensure_members(dbgk_inf *z, uint64_t n)
{
	if (n > z->cap_members || !z->off) {
		z->cap_members = 0;
		const uint64_t cap = std::max<uint64_t>(n, 1024);
		if (z->off.reserve((cap + 1) * 8) || z->place.reserve((cap + 1) * 8) || z->isize.reserve((cap + 1) * 4) || z->crc.reserve(cap * 4) ||
		    z->status.reserve(cap * 4))
			return DBGK_ERR_NOMEM;
		z->cap_members = cap;
	}
	const uint64_t round = std::min<uint64_t>(n, infk::kInfRound);
	if (round > z->cap_round || !z->tokens) {
		z->cap_round = 0;
		const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(round, 64), infk::kInfRound);
		if (z->tokens.reserve(cap * gzf::kGzPiece * 4) || z->n_tok.reserve(cap * 4)) return DBGK_ERR_NOMEM;
		z->cap_round = cap;
	}
	return DBGK_OK;
}

// members that lie on the device, complete: the handle's stream is non-blocking and waits for no work of the caller's (dbgk_inf_inflate
// has synchronised its upload; dbgk_inf_inflate_device leaves that to the caller).  off: the host's table, n + 1 entries, checked.
static int inf_run(dbgk_inf *z, const uint8_t *gz, const uint64_t *off, uint64_t n, dbgk_inf_info *info)
{
	z->have = false;
	dbgk_inf_info I{};
	dbgk_inf_timing T{};
	I.n_members = n;
	I.consumed = n ? off[n] : 0;
	z->reasons.assign(n, 0);
	if (n) {
		int rc = inf_ensure_members(z, n);
		if (rc) return rc;
		const uint32_t nm = (uint32_t)n;
		HIPCHK(hipMemcpyAsync(z->off, off, (n + 1) * 8, hipMemcpyHostToDevice, z->stream));
		HIPCHK(hipMemsetAsync(z->ctr, 0, infk::IC_COUNT * 8, z->stream));
		rc = stage_scan_reserve(z->tmp, z->stream, z->isize, z->place, n + 1);
		if (rc) return rc;
		HIPCHK(hipEventRecord(z->ev[0], z->stream));
		hipLaunchKernelGGL(infk::k_inf_sizes, dim3(nm / infk::kInfBlock + 1), dim3(infk::kInfBlock), 0, z->stream, gz, (const uint64_t *)z->off, nm, z->isize, z->crc,
		                   z->status, z->ctr);
		HIPCHK(hipGetLastError());
		rc = stage_scan(z->tmp, z->stream, z->isize, z->place, n + 1);
		if (rc) return rc;
		HIPCHK(hipEventRecord(z->ev[1], z->stream));
		uint64_t total = 0;
		HIPCHK(hipMemcpyAsync(&total, z->place + n, 8, hipMemcpyDeviceToHost, z->stream));
		HIPCHK(hipStreamSynchronize(z->stream)); // the total sizes the output
		if (total > z->max_out) {
			g_last_error = "the members inflate to more than max_out_bytes";
			return DBGK_ERR_ARG;
		}
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, z->ev[0], z->ev[1]));
		T.ms_scan = ms;
		if (z->out.reserve(total + 16, 1 << 20)) return DBGK_ERR_NOMEM;
		for (uint32_t r0 = 0; r0 < nm; r0 += infk::kInfRound) {
			const uint32_t nr = std::min<uint32_t>(nm - r0, infk::kInfRound);
			HIPCHK(hipEventRecord(z->ev[0], z->stream));
			hipLaunchKernelGGL(infk::k_inf_decode, dim3((nr + infk::kInfLanes - 1) / infk::kInfLanes), dim3(infk::kInfDecodeBlock), 0, z->stream, gz,
			                   (const uint64_t *)z->off, (const uint32_t *)z->isize, r0, nr, z->tokens, z->n_tok, z->status, z->ctr);
			HIPCHK(hipGetLastError());
			HIPCHK(hipEventRecord(z->ev[1], z->stream));
			hipLaunchKernelGGL(infk::k_inf_resolve, dim3(nr), dim3(infk::kInfBlock), sizeof(infk::InfResolveLds), z->stream, (const uint32_t *)z->tokens,
			                   (const uint32_t *)z->n_tok, (const uint32_t *)z->isize, (const uint32_t *)z->crc, (const uint64_t *)z->place, (const uint32_t *)z->x8, r0,
			                   z->status, z->out);
			HIPCHK(hipGetLastError());
			HIPCHK(hipEventRecord(z->ev[2], z->stream));
			HIPCHK(hipStreamSynchronize(z->stream)); // the next round writes the token area again
			HIPCHK(hipEventElapsedTime(&ms, z->ev[0], z->ev[1]));
			T.ms_decode += ms;
			HIPCHK(hipEventElapsedTime(&ms, z->ev[1], z->ev[2]));
			T.ms_resolve += ms;
		}
		std::vector<uint32_t> status(n);
		unsigned long long ctr[infk::IC_COUNT] = {0};
		HIPCHK(hipMemcpyAsync(status.data(), z->status, n * 4, hipMemcpyDeviceToHost, z->stream));
		HIPCHK(hipMemcpyAsync(ctr, z->ctr, sizeof ctr, hipMemcpyDeviceToHost, z->stream));
		HIPCHK(hipStreamSynchronize(z->stream));
		for (uint64_t m = 0; m < n; ++m) {
			z->reasons[m] = (uint8_t)status[m];
			if (!status[m]) continue;
			if (!I.n_bad) I.first_bad = m, I.first_bad_reason = status[m];
			I.n_bad++;
		}
		I.out_bytes = total;
		I.n_markers = ctr[infk::IC_MARKERS];
		I.n_stored = ctr[infk::IC_STORED];
		I.n_fixed = ctr[infk::IC_FIXED];
		I.n_dynamic = ctr[infk::IC_DYNAMIC];
		I.n_literals = ctr[infk::IC_LITERALS];
		I.n_matches = ctr[infk::IC_MATCHES];
	}
	z->info = I;
	z->timing = T;
	z->have = true;
	if (info) *info = I;
	return DBGK_OK;
}

extern "C" int dbgk_inf_inflate_device(dbgk_inf *z, const void *d_gz, uint64_t n_bytes, const uint64_t *member_offsets, uint64_t n_members,
                                       dbgk_inf_info *info)
{
	if (!z || n_bytes >= (1ull << 31) || (n_bytes && !d_gz) || ((uintptr_t)d_gz & 15u) || !member_offsets || n_members >= (1ull << 31)) return DBGK_ERR_ARG;
	for (uint64_t m = 0; m < n_members; ++m)
		if (member_offsets[m + 1] < member_offsets[m]) return DBGK_ERR_ARG;
	if (member_offsets[n_members] > n_bytes) return DBGK_ERR_ARG;
	const uint8_t *u = (const uint8_t *)d_gz;
	if (u && z->out && u + n_bytes > z->out && u < z->out + z->out.cap) return DBGK_ERR_ARG; // the output the call is about to write
	HIPCHK(hipSetDevice(z->device));
	return inf_run(z, u, member_offsets, n_members, info);
}

extern "C" int dbgk_inf_inflate(dbgk_inf *z, const void *gz, uint64_t n_bytes, int last, dbgk_inf_info *info)
{
	if (!z || n_bytes >= (1ull << 31) || (n_bytes && !gz)) return DBGK_ERR_ARG;
	z->have = false;
	static const char *const why[] = {"", "a member is cut short", "not the 16 fixed header bytes of a BGZF member", "a BSIZE too small to hold header and trailer",
	                                  "an ISIZE above 65280"};
	const uint8_t *buf = (const uint8_t *)gz;
	uint64_t count = 0;
	const int rc = gzf::gz_frame_walk(buf, n_bytes, nullptr, 0, &count, nullptr);
	if (rc > 1 || (rc == 1 && last)) {
		g_last_error = std::string("dbgk_inf_inflate: ") + why[rc];
		return DBGK_ERR_ARG;
	}
	std::vector<gzf::GzMember> ms(count);
	(void)gzf::gz_frame_walk(buf, n_bytes, ms.data(), count, &count, nullptr);
	// whole members from the front while their bytes stay within max_out
	std::vector<uint64_t> off;
	off.reserve(count + 1);
	off.push_back(0);
	uint64_t sum = 0;
	for (uint64_t m = 0; m < count; ++m) {
		if (sum + ms[m].isize > z->max_out) break;
		sum += ms[m].isize;
		off.push_back(ms[m].offset + ms[m].size);
	}
	const uint64_t n = off.size() - 1, used = off[n];
	HIPCHK(hipSetDevice(z->device));
	if (used + 16 > z->gz.cap) {
		HIPCHK(hipStreamSynchronize(z->stream));
		if (z->gz.reserve(used + 16, 1 << 20)) return DBGK_ERR_NOMEM;
	}
	if (used) HIPCHK(hipMemcpyAsync(z->gz, gz, used, hipMemcpyHostToDevice, z->stream));
	HIPCHK(hipStreamSynchronize(z->stream)); // the caller's buffer is free on return
	return inf_run(z, z->gz, off.data(), n, info);
}

extern "C" int dbgk_inf_results(dbgk_inf *z, void *out, uint64_t capacity)
{
	if (!z) return DBGK_ERR_ARG;
	if (!z->have) return DBGK_ERR_STATE;
	if (capacity < z->info.out_bytes || (z->info.out_bytes && !out)) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(z->device));
	if (z->info.out_bytes) HIPCHK(hipMemcpyAsync(out, z->out, z->info.out_bytes, hipMemcpyDeviceToHost, z->stream));
	HIPCHK(hipStreamSynchronize(z->stream));
	return DBGK_OK;
}

extern "C" int dbgk_inf_device(dbgk_inf *z, const void **d_text, uint64_t *n_bytes)
{
	if (!z || !d_text || !n_bytes) return DBGK_ERR_ARG;
	if (!z->have) return DBGK_ERR_STATE;
	*d_text = z->info.out_bytes ? z->out.p : nullptr;
	*n_bytes = z->info.out_bytes;
	return DBGK_OK;
}

extern "C" int dbgk_inf_member_status(dbgk_inf *z, uint8_t *reason, uint64_t capacity)
{
	if (!z) return DBGK_ERR_ARG;
	if (!z->have) return DBGK_ERR_STATE;
	if (capacity < z->reasons.size() || (!z->reasons.empty() && !reason)) return DBGK_ERR_ARG;
	if (!z->reasons.empty()) memcpy(reason, z->reasons.data(), z->reasons.size());
	return DBGK_OK;
}

extern "C" int dbgk_inf_timing_get(dbgk_inf *z, dbgk_inf_timing *t)
{
	if (!z || !t) return DBGK_ERR_ARG;
	*t = z->timing;
	return DBGK_OK;
}
