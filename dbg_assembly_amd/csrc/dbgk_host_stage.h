// What every handle is built from -- the graph handle (dbgk_handle) and the stage handles (CORRECT, MAP, CLEAN, PAIR, PARSE, FORMAT,
// DEFLATE, INFLATE, LINK, CONTIG, and the buffers of FILL and SUPER): the device it runs on with its stream, device and pinned buffers
// that free themselves, events, further streams, and the scan's temporary storage.  A handle derives from StageDev, so the stream is
// made first and destroyed last: it outlives every buffer and event the handle owns.  A *_destroy is then: null check, stage_drain,
// the handle's own waits, delete.  Host functions hold their temporaries in the same owners: every return path frees them.

// dbgk_sort.hip
extern "C" int dbgk_internal_scan_lengths(void *tmp, size_t *tmp_bytes, const uint32_t *d_len, uint64_t *d_offsets, uint64_t n_items,
                                          hipStream_t stream);

constexpr int kStageCurrentDevice = -1; // stage_open: the device that is current on the calling thread (0 when none can be read)

// the device's stream is idle and the device current: what a *_destroy does before it deletes the handle
static void stage_drain(int device, hipStream_t stream)
{
	if (!stream) return;
	(void)hipSetDevice(device);
	(void)hipStreamSynchronize(stream);
}

struct StageDev {
	int device = 0;
	int n_cu = 256;
	hipStream_t stream = nullptr;
	StageDev() = default;
	StageDev(const StageDev &) = delete;
	StageDev &operator=(const StageDev &) = delete;
	~StageDev()
	{
		stage_drain(device, stream);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

// The device `device` (or kStageCurrentDevice) made current, checked to be a gfx950, its CU count, and a non-blocking stream on it.
// The caller has checked its own arguments, `device >= 0` among them, before this first HIP call.
static int stage_open(StageDev &d, int device)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || (device == kStageCurrentDevice ? n_dev < 1 : device >= n_dev)) {
		g_last_error = "no usable HIP device";
		return DBGK_ERR_HIP;
	}
	if (device == kStageCurrentDevice && hipGetDevice(&device) != hipSuccess) device = 0;
	d.device = device;
	hipDeviceProp_t prop;
	if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) return DBGK_ERR_HIP;
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		g_last_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
		return DBGK_ERR_HIP;
	}
	d.n_cu = prop.multiProcessorCount;
	if (hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess) return DBGK_ERR_HIP;
	return DBGK_OK;
}

// N events of a handle, e.g. the two ends of each span it times
template <int N>
struct StageEvents {
	hipEvent_t e[N] = {};
	StageEvents() = default;
	StageEvents(const StageEvents &) = delete;
	StageEvents &operator=(const StageEvents &) = delete;
	~StageEvents()
	{
		for (hipEvent_t x : e)
			if (x) (void)hipEventDestroy(x);
	}
	int create()
	{
		for (hipEvent_t &x : e)
			if (hipEventCreate(&x) != hipSuccess) return DBGK_ERR_HIP;
		return DBGK_OK;
	}
	hipEvent_t operator[](int i) const { return e[i]; }
};

// One event, made when it is first needed.  It moves, so it can live in a std::vector.
struct StageEvent {
	hipEvent_t e = nullptr;
	StageEvent() = default;
	StageEvent(StageEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
	StageEvent &operator=(StageEvent &&o) noexcept
	{
		std::swap(e, o.e);
		return *this;
	}
	~StageEvent()
	{
		if (e) (void)hipEventDestroy(e);
	}
	operator hipEvent_t() const { return e; }
	int create(unsigned flags = hipEventDefault)
	{
		if (!e) HIPCHK(hipEventCreateWithFlags(&e, flags));
		return DBGK_OK;
	}
};

// A stream beside the handle's first one, made when it is first needed.  Its owner drains it before the handle goes.
struct StageStream {
	hipStream_t s = nullptr;
	StageStream() = default;
	StageStream(const StageStream &) = delete;
	StageStream &operator=(const StageStream &) = delete;
	~StageStream()
	{
		if (s) (void)hipStreamDestroy(s);
	}
	operator hipStream_t() const { return s; }
	int create()
	{
		if (!s) HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
		return DBGK_OK;
	}
};

// A device buffer and its size in bytes.  It converts to its pointer, so launches, copies and pointer arithmetic read as
// they do with a plain pointer; where a cast or a `? :` needs the pointer itself, it is `.p`.
template <class T>
struct DevBuf {
	T *p = nullptr;
	uint64_t cap = 0; // bytes
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	DevBuf(DevBuf &&o) noexcept { take(o); }
	DevBuf &operator=(DevBuf &&o) noexcept // (a struct of buffers is emptied by assigning a fresh one)
	{
		take(o);
		return *this;
	}
	~DevBuf() { release(); }
	operator T *() const { return p; }
	T *operator->() const { return p; }
	void release()
	{
		(void)hipFree(p);
		p = nullptr;
		cap = 0;
	}
	// At least `want` bytes: a buffer that has them stays, else it is freed and one of max(want, floor) bytes made.  The content is NOT
	// kept, and nothing queued may still read the old buffer.  On failure the buffer is empty.
	int reserve(uint64_t want, uint64_t floor = 0)
	{
		if (p && want <= cap) return DBGK_OK;
		release();
		const uint64_t n = std::max(want, floor);
		if (hipMalloc(&p, n) != hipSuccess) {
			p = nullptr;
			return DBGK_ERR_NOMEM;
		}
		cap = n;
		return DBGK_OK;
	}
	// the buffer of `other`, which is left empty (the copy-then-swap of a grow that keeps its content)
	void take(DevBuf &other)
	{
		release();
		p = other.p;
		cap = other.cap;
		other.p = nullptr;
		other.cap = 0;
	}
};

// A page-locked host buffer.  Like DevBuf it converts to its pointer; it moves, so it can live in a std::vector.
template <class T>
struct PinBuf {
	T *p = nullptr;
	PinBuf() = default;
	PinBuf(PinBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
	PinBuf &operator=(PinBuf &&o) noexcept
	{
		std::swap(p, o.p);
		return *this;
	}
	~PinBuf()
	{
		if (p) (void)hipHostFree(p);
	}
	operator T *() const { return p; }
	T *operator->() const { return p; }
	int alloc(uint64_t bytes) // (an empty buffer only)
	{
		if (hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) return DBGK_OK;
		p = nullptr;
		return DBGK_ERR_NOMEM;
	}
};

// the temporary storage of dbgk_internal_scan_lengths
struct ScanTmp {
	DevBuf<uint8_t> buf;
};

// room for a scan of n_items values.  When the storage has to grow the stream is drained first: a scan queued earlier may still use it.
static int stage_scan_reserve(ScanTmp &t, hipStream_t stream, const uint32_t *in, uint64_t *out, uint64_t n_items)
{
	size_t need = 0;
	if (dbgk_internal_scan_lengths(nullptr, &need, in, out, n_items, stream)) return DBGK_ERR_HIP;
	if (need <= t.buf.cap) return DBGK_OK;
	HIPCHK(hipStreamSynchronize(stream));
	return t.buf.reserve(need);
}

// an exclusive scan of n_items 32-bit values into 64-bit offsets, queued on `stream`
static int stage_scan(ScanTmp &t, hipStream_t stream, const uint32_t *in, uint64_t *out, uint64_t n_items)
{
	const int rc = stage_scan_reserve(t, stream, in, out, n_items);
	if (rc) return rc;
	size_t bytes = t.buf.cap;
	return dbgk_internal_scan_lengths(t.buf, &bytes, in, out, n_items, stream) ? DBGK_ERR_HIP : DBGK_OK;
}
