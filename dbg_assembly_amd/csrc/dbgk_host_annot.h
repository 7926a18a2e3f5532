// ANNOT, host side (include/dbgk.h, CORRECT section; kernels in dbgk_annot.h): the suffix plane of a corrector's compact batch on the
// device.  dbgk_corr holds one AnnotStage; the C entries are at the end of dbgk_host_correct.h.

struct AnnotStage {
	DevBuf<uint8_t> suf;  // 16-byte vectors, the pad of the last one 0, 64 readable bytes behind
	DevBuf<uint64_t> off; // n + 1 suffix offsets
	DevBuf<uint32_t> len;
	uint64_t cap_recs = 0;
	ScanTmp tmp;
	uint64_t n = 0, total = 0;
	bool have = false;    // the plane belongs to the handle's current compact batch
	StageEvents<4> ev;    // length + scan: [0] .. [1]; write: [2] .. [3]
};

// rec, coff: the n records and the n + 1 compact offsets of the batch, on the device and complete
static int annot_run(AnnotStage &s, hipStream_t stream, int n_cu, const dbgk_corr_rec *rec, const uint64_t *coff, uint64_t n, dbgk_corr_annot_info *out)
{
	s.have = false;
	if (n >= (1ull << 32)) return DBGK_ERR_ARG;
	if (n + 1 > s.cap_recs || !s.off || !s.len) {
		const uint64_t cap = std::max<uint64_t>(n + 1, 1 << 14);
		s.cap_recs = 0;
		if (s.off.reserve(cap * 8) || s.len.reserve(cap * 4)) return DBGK_ERR_NOMEM;
		s.cap_recs = cap;
	}
	int rc = DBGK_OK;
	if (n && (rc = stage_scan_reserve(s.tmp, stream, s.len, s.off, n + 1))) return rc;
	HIPCHK(hipEventRecord(s.ev[0], stream));
	if (n) {
		const unsigned grid = (unsigned)std::min<uint64_t>((n + emitk::kEmitBlock) / emitk::kEmitBlock, (uint64_t)n_cu * 16);
		hipLaunchKernelGGL(annotk::k_annot_len, dim3(grid), dim3(emitk::kEmitBlock), 0, stream, rec, coff, (uint32_t)n, s.len);
		HIPCHK(hipGetLastError());
		if ((rc = stage_scan(s.tmp, stream, s.len, s.off, n + 1))) return rc;
	} else {
		HIPCHK(hipMemsetAsync(s.off, 0, 8, stream));
	}
	HIPCHK(hipEventRecord(s.ev[1], stream));
	uint64_t total = 0;
	HIPCHK(hipMemcpyAsync(&total, s.off + n, 8, hipMemcpyDeviceToHost, stream));
	HIPCHK(hipStreamSynchronize(stream)); // the total sizes the plane
	if (total > n * annotk::kAnnotMax) return DBGK_ERR_HIP; // (never: the bound of a suffix is the LDS span of the write kernel)
	if (s.suf.reserve(((total + 15) & ~15ull) + 64, 1 << 20)) return DBGK_ERR_NOMEM;
	if (total) {
		const uint64_t groups = (n + annotk::kAnnotGroup - 1) / annotk::kAnnotGroup;
		const unsigned grid = (unsigned)std::min<uint64_t>(groups, (uint64_t)n_cu * 5); // (five workgroups' LDS per CU)
		HIPCHK(hipEventRecord(s.ev[2], stream));
		hipLaunchKernelGGL(annotk::k_annot_write, dim3(grid), dim3(emitk::kEmitBlock), 0, stream, rec, coff, (const uint64_t *)s.off, (uint32_t)n,
		                   reinterpret_cast<uint4 *>(s.suf.p));
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(s.ev[3], stream));
		HIPCHK(hipStreamSynchronize(stream));
	}
	dbgk_corr_annot_info I{};
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
	I.ms_scan = ms;
	if (total) {
		HIPCHK(hipEventElapsedTime(&ms, s.ev[2], s.ev[3]));
		I.ms_write = ms;
	}
	I.n = n;
	I.suffix_bytes = total;
	s.n = n;
	s.total = total;
	s.have = true;
	*out = I;
	return DBGK_OK;
}
