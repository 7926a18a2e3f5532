// DEFLATE stage, host side (include/dbgk.h, GZ section; kernels in dbgk_gz.h, framing in dbgk_gz_frame.h).  One call is three
// launches on the handle's stream -- members, the scan of their sizes, the gather -- and one read-back of the total in between,
// which sizes the output.  Calls are stateless: nothing but the buffers outlives one.

struct dbgk_gz : StageDev {
	int level = 1;
	DevBuf<uint8_t> text; // dbgk_gz_deflate: the uploaded text
	DevBuf<uint32_t> slots; // cap_slots slots of kGzSlot bytes
	DevBuf<uint32_t> sizes; // cap_slots + 1
	DevBuf<uint32_t> tokens; // level 2: kGzPiece tokens per slot
	DevBuf<uint64_t> off;
	uint64_t cap_slots = 0;
	DevBuf<uint8_t> out;
	ScanTmp tmp; // the scan's
	DevBuf<uint32_t> x8;
	DevBuf<unsigned long long> ctr;
	StageEvents<4> ev; // members, scan + gather
	bool have = false;
	dbgk_gz_info info{};
	dbgk_gz_timing timing{};
};

extern "C" int dbgk_gz_destroy(dbgk_gz *z)
{
	if (!z) return DBGK_ERR_ARG;
	stage_drain(z->device, z->stream);
	delete z;
	return DBGK_OK;
}

// the member kernel's LDS is above 64 KiB
static int gz_raise_lds()
{
	DBGK_LDS_ATTR(gzk::k_gz_members, sizeof(gzk::GzLds));
	return DBGK_OK;
}

extern "C" int dbgk_gz_create(int level, dbgk_gz **out)
{
	if (!out) return DBGK_ERR_ARG;
	*out = nullptr;
	if (level < 0 || level > DBGK_GZ_MAX_LEVEL) return DBGK_ERR_ARG;
	dbgk_gz *z = new (std::nothrow) dbgk_gz;
	if (!z) return DBGK_ERR_NOMEM;
	z->level = level;
	int rc = stage_open(*z, kStageCurrentDevice);
	if (!rc) rc = z->ev.create();
	if (!rc && (z->x8.reserve(16 * 4) || z->ctr.reserve(gzk::GC_COUNT * 8))) rc = DBGK_ERR_NOMEM;
	if (!rc) {
		const gzf::GzPowers t = gzf::gz_powers();
		if (hipMemcpy(z->x8, t.x8, 16 * 4, hipMemcpyHostToDevice) != hipSuccess) rc = DBGK_ERR_HIP;
	}
	if (!rc) rc = gz_raise_lds();
	if (rc) {
		dbgk_gz_destroy(z);
		return rc;
	}
	*out = z;
	return DBGK_OK;
}

// (the stream is idle)
static int gz_ensure_slots(dbgk_gz *z, uint64_t n_slots)
{
	if (n_slots <= z->cap_slots && z->slots) return DBGK_OK;
	z->cap_slots = 0;
	const uint64_t cap = std::max<uint64_t>(n_slots, 64);
	if (z->slots.reserve(cap * gzf::kGzSlot) || z->sizes.reserve((cap + 1) * 4) || z->off.reserve((cap + 1) * 8) ||
	    (z->level == 2 && z->tokens.reserve(cap * gzf::kGzPiece * 4)))
		return DBGK_ERR_NOMEM;
	z->cap_slots = cap;
	return DBGK_OK;
}

// text that lies on the device, readable up to n_bytes rounded up to 16 (the stream is ordered behind whatever wrote it)
static int gz_run(dbgk_gz *z, const uint8_t *text, uint64_t n_bytes, bool last, dbgk_gz_info *info)
{
	z->have = false;
	const uint32_t nb = (uint32_t)n_bytes, n_members = (nb + gzf::kGzPiece - 1) / gzf::kGzPiece, n_slots = n_members + (last ? 1u : 0u);
	dbgk_gz_info I{};
	dbgk_gz_timing T{};
	I.n_members = n_members;
	if (n_slots) {
		int rc = gz_ensure_slots(z, n_slots);
		if (rc) return rc;
		HIPCHK(hipMemsetAsync(z->ctr, 0, gzk::GC_COUNT * 8, z->stream));
		HIPCHK(hipEventRecord(z->ev[0], z->stream));
		hipLaunchKernelGGL(gzk::k_gz_members, dim3(std::min<uint32_t>(n_slots, (uint32_t)z->n_cu * 8)), dim3(gzk::kGzBlock),
		                   z->level == 2 ? sizeof(gzk::GzLds) : offsetof(gzk::GzLds, M), z->stream,
		                   reinterpret_cast<const uint4 *>(text), nb, n_members, n_slots, (uint32_t)z->level, (const uint32_t *)z->x8, z->slots, z->sizes,
		                   z->tokens, z->ctr);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(z->ev[1], z->stream));
		rc = stage_scan_reserve(z->tmp, z->stream, z->sizes, z->off, (uint64_t)n_slots + 1);
		if (rc) return rc;
		HIPCHK(hipEventRecord(z->ev[2], z->stream));
		rc = stage_scan(z->tmp, z->stream, z->sizes, z->off, (uint64_t)n_slots + 1);
		if (rc) return rc;
		uint64_t total = 0;
		unsigned long long ctr[gzk::GC_COUNT] = {0};
		HIPCHK(hipMemcpyAsync(&total, z->off + n_slots, 8, hipMemcpyDeviceToHost, z->stream));
		HIPCHK(hipMemcpyAsync(ctr, z->ctr, sizeof ctr, hipMemcpyDeviceToHost, z->stream));
		HIPCHK(hipStreamSynchronize(z->stream)); // the total sizes the output
		if (total > (uint64_t)n_slots * gzf::kGzSlot) {
			g_last_error = "member sizes exceed their slots";
			return DBGK_ERR_STATE;
		}
		if (z->out.reserve(total + 16, 1 << 20)) return DBGK_ERR_NOMEM;
		hipLaunchKernelGGL(gzk::k_gz_gather, dim3(std::min<uint32_t>(n_slots, (uint32_t)z->n_cu * 16)), dim3(gzk::kGzBlock), 0, z->stream,
		                   reinterpret_cast<const uint8_t *>(z->slots.p), (const uint64_t *)z->off, n_slots, z->out);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(z->ev[3], z->stream));
		HIPCHK(hipStreamSynchronize(z->stream));
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, z->ev[0], z->ev[1]));
		T.ms_members = ms;
		HIPCHK(hipEventElapsedTime(&ms, z->ev[2], z->ev[3]));
		T.ms_compact = ms;
		I.out_bytes = total;
		I.stored_members = ctr[gzk::GC_STORED];
		I.n_literals = ctr[gzk::GC_LITERALS];
		I.n_matches = ctr[gzk::GC_MATCHES];
		I.match_bytes = ctr[gzk::GC_MATCH_BYTES];
		// the launch's time by the phases' shares of the cycles lane 0 of every workgroup counted
		const double cyc = (double)ctr[gzk::GC_CYC_MATCH] + (double)ctr[gzk::GC_CYC_HIST] + (double)ctr[gzk::GC_CYC_CODES] + (double)ctr[gzk::GC_CYC_ENCODE];
		if (cyc > 0) {
			T.ms_match = T.ms_members * (double)ctr[gzk::GC_CYC_MATCH] / cyc;
			T.ms_crc_hist = T.ms_members * (double)ctr[gzk::GC_CYC_HIST] / cyc;
			T.ms_codes = T.ms_members * (double)ctr[gzk::GC_CYC_CODES] / cyc;
			T.ms_encode = T.ms_members * (double)ctr[gzk::GC_CYC_ENCODE] / cyc;
		}
	}
	z->info = I;
	z->timing = T;
	z->have = true;
	if (info) *info = I;
	return DBGK_OK;
}

extern "C" int dbgk_gz_deflate_device(dbgk_gz *z, const void *d_text, uint64_t n_bytes, int last, dbgk_gz_info *info)
{
	if (!z || n_bytes >= (1ull << 31) || (n_bytes && !d_text) || ((uintptr_t)d_text & 15u)) return DBGK_ERR_ARG;
	const uint8_t *u = (const uint8_t *)d_text;
	if (u && z->out && u + n_bytes > z->out && u < z->out + z->out.cap) return DBGK_ERR_ARG; // the output the call is about to write
	HIPCHK(hipSetDevice(z->device));
	return gz_run(z, u, n_bytes, last != 0, info);
}

extern "C" int dbgk_gz_deflate(dbgk_gz *z, const void *text, uint64_t n_bytes, int last, dbgk_gz_info *info)
{
	if (!z || n_bytes >= (1ull << 31) || (n_bytes && !text)) return DBGK_ERR_ARG;
	z->have = false;
	HIPCHK(hipSetDevice(z->device));
	if (n_bytes + 16 > z->text.cap) {
		HIPCHK(hipStreamSynchronize(z->stream));
		if (z->text.reserve(n_bytes + 16, 1 << 20)) return DBGK_ERR_NOMEM;
	}
	if (n_bytes) HIPCHK(hipMemcpyAsync(z->text, text, n_bytes, hipMemcpyHostToDevice, z->stream));
	HIPCHK(hipStreamSynchronize(z->stream)); // the caller's buffer is free on return
	return gz_run(z, z->text, n_bytes, last != 0, info);
}

extern "C" int dbgk_gz_results(dbgk_gz *z, void *out, uint64_t capacity)
{
	if (!z) return DBGK_ERR_ARG;
	if (!z->have) return DBGK_ERR_STATE;
	if (capacity < z->info.out_bytes || (z->info.out_bytes && !out)) return DBGK_ERR_ARG;
	HIPCHK(hipSetDevice(z->device));
	if (z->info.out_bytes) HIPCHK(hipMemcpyAsync(out, z->out, z->info.out_bytes, hipMemcpyDeviceToHost, z->stream));
	HIPCHK(hipStreamSynchronize(z->stream));
	return DBGK_OK;
}

extern "C" int dbgk_gz_device(dbgk_gz *z, const void **d_out, uint64_t *n_out)
{
	if (!z || !d_out || !n_out) return DBGK_ERR_ARG;
	if (!z->have) return DBGK_ERR_STATE;
	*d_out = z->info.out_bytes ? z->out.p : nullptr;
	*n_out = z->info.out_bytes;
	return DBGK_OK;
}

extern "C" int dbgk_gz_timing_get(dbgk_gz *z, dbgk_gz_timing *t)
{
	if (!z || !t) return DBGK_ERR_ARG;
	*t = z->timing;
	return DBGK_OK;
}
