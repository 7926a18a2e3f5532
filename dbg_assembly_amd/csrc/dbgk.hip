// dbgk.hip -- host side of the C ABI declared in include/dbgk.h: device memory, stream, staging,
// kernel launches.  gfx950 only; no CPU fallback.
#define DBGK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <chrono>
#include <cmath>
#include <emmintrin.h>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "dbgk.h"
#include "dbgk_env.h"
#include "dbgk_kernels.h"
#include "dbgk_partition.h"
#include "dbgk_wide_kernels.h"
#include "dbgk_wide_links_patch.h"
#include "dbgk_wide_partition.h"
#include "dbgk_correct.h"
#include "dbgk_spectrum.h"
#include "dbgk_map.h"
#include "dbgk_clean.h"
#include "dbgk_emit.h"
#include "dbgk_pair.h"
#include "dbgk_parse.h"
#include "dbgk_format.h"
#include "dbgk_annot.h"
#include "dbgk_maprow.h"
#include "dbgk_gz.h"
#include "dbgk_inflate.h"
#include "dbgk_link.h"
#include "dbgk_fill.h"
#include "dbgk_super.h"
#include "dbgk_contig.h"
#include "dbgk_wide_contig.h"
#include "dbgk_simplify.h"
#include "dbgk_wide_simplify.h"
#include "dbgk_align.h"
#include "dbgk_l1_form.h"

// dbgk_sort.hip
extern "C" int dbgk_internal_sort_pairs(uint64_t *d_keys, uint64_t *d_vals, uint64_t n, hipStream_t stream);

using namespace dbgk;

static_assert(sizeof(dbgk_node) == 16 && sizeof(Node) == 16, "node layout must match KmerNode (kmerSet.h:70-75)");

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int hip_fail(hipError_t e, const char *what, int line)
{
	char buf[512];
	snprintf(buf, sizeof buf, "%s failed at dbgk.hip:%d: %s", what, line, hipGetErrorString(e));
	g_last_error = buf;
	return DBGK_ERR_HIP;
}

#define HIPCHK(expr)                                                   \
	do {                                                               \
		hipError_t e__ = (expr);                                       \
		if (e__ != hipSuccess) return hip_fail(e__, #expr, __LINE__);  \
	} while (0)

#include "dbgk_host_stage.h"

// ---------------------------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t kMaxBuildLaunches = 4096; // build ranges per step (one work cursor each)
constexpr uint64_t kHeavyHitterSlots = 4194301; // side table for the surplus of heavy hitters (prime, 64 MiB)

enum Phase { PH_MARK = 0, PH_INSERT, PH_PARTITION, PH_BUILD, PH_FIXUP, PH_FINALIZE, PH_L2_BUILD_WALL, PH_COUNT };

struct TimedSpan {
	StageEvent a, b;
	int phase = 0;
};

struct StageSlot {
	PinBuf<char> h_bases;
	PinBuf<uint64_t> h_offsets;
	DevBuf<char> d_bases;
	DevBuf<uint64_t> d_offsets;
	DevBuf<uint32_t> d_start;
	DevBuf<uint32_t> d_dead;
	StageEvent done;                // the kernels that read the device buffers have run
	StageEvent copied;              // the host-to-device copies of the batch have run (copy stream)
	bool busy = false;
	bool acquired = false;          // handed out by dbgk_push_acquire and not committed yet
};

// What owns the memory behind the PartStore / WPartStore views that the kernels take (setup_partition, setup_wide_partition fill
// the views).  A resize re-makes the stores: it assigns a fresh one.
struct PartBufs {
	DevBuf<uint64_t> l1, l2, inbox, mid;
	DevBuf<uint32_t> cnt1, cnt2, inbox_cnt, cnt_mid;
	DevBuf<Node> ovf, spill, hh, outgoing;
	DevBuf<unsigned long long> ovf_n, outgoing_n;
	DevBuf<uint32_t> tile_prefix;    // [n_ranks * B + 1] level-2 tile plan
	DevBuf<uint32_t> tile_prefix2;   // [nb_own * fan_mid + 1]
	DevBuf<uint32_t> l2_done;        // EARLY level 2 (early_l2): records per level-1 bucket that level 2 has taken already; null = not in use
	DevBuf<unsigned int> region_cursor; // [kMaxBuildLaunches] work cursors of the persistent build launches
};

struct WPartBufs {
	DevBuf<ull2> l1, l2, inbox;      // inbox, sharded: [n_l1][cap1] records of my buckets from every rank
	DevBuf<uint32_t> cnt1, cnt2, inbox_cnt, tile_prefix;
	DevBuf<dbgk_node32> ovf, spill, outgoing;
	DevBuf<unsigned long long> ovf_n, outgoing_n;
	DevBuf<unsigned int> cursor;
	DevBuf<dbgk_node32> side_out;    // [kWideSideSlots + 1] dbgk_shard_side_export
	DevBuf<unsigned long long> side_n;
};

// what plan_partition decides for a configuration and a modulus: engine, shard, and the geometry of its record stores
struct PartPlan {
	bool part = false, sharded = false, three = false;
	uint32_t fan_mid = 0, shard_rank = 0;
	uint64_t tslots = 0;
	PartGeom geom, g_mid, g_fin;
};

} // namespace

struct dbgk_handle : StageDev {
	dbgk_config cfg;
	int grid = 2048;

	DevBuf<Node> table;
	uint64_t size = 0;            // hash modulus: slot = hash_code(key) % size (the GLOBAL table when sharded)
	uint64_t tslots = 0;          // slots held by `table` (== size unless sharded)
	ModMagic magic;

	DevBuf<Counters> d_ctr;
	PinBuf<Counters> h_ctr;

	// host-buffer staging
	StageSlot slots[2];
	uint64_t cap_bases = 0, cap_reads = 0;
	int next_slot = 0;

	// bitmaps for the device-pointer path
	DevBuf<uint32_t> dev_start, dev_dead;
	// level 1 for reads of any lengths (k_extract_scatter_prefix): the per-read lane prefix of the current batch, and the
	// 2-bit form of a batch that came as ASCII.  One set per handle: batches follow each other on one stream.
	DevBuf<ReadLanes> pf_ent;
	DevBuf<uint32_t> pf_tile_first;
	DevBuf<PrefixTile> pf_tiles;
	DevBuf<unsigned long long> pf_bsum;
	DevBuf<PrefixTotals> pf_tot;
	DevBuf<uint32_t> pf_packed;
	DevBuf<uint64_t> uni_offsets; // offsets made on the device for a batch that came without (dbgk_push_reads_packed_uniform*) and needs them
	uint32_t prefix_launches = 0;

	bool finalized = false;
	uint64_t total_reads = 0;
	uint64_t host_other_bytes = 0; // bytes outside ACGTNacgtn that a host packer met (dbgk_push_reads_packed / dbgk_push_commit_packed)

	// first-seen tracking (DBGK_FLAG_TRACK_FIRST_SEEN, DIRECT engine)
	bool track = false;
	DevBuf<unsigned long long> first_pos;    // [tslots]
	uint64_t pos_base = 0;                   // bases pushed so far

	bool wide = false;            // WIDE engine: 128-bit keys, 32-byte nodes (dbgk_wide_kernels.h)
	DevBuf<WNode> wnodes;         // [size]
	DevBuf<WNode> wside;          // [kWideSideSlots]
	// WIDE through radix-partitioned records (dbgk_wide_partition.h): expected_kmers > 0 and a feasible geometry
	bool wpart = false;
	bool wbuilt = false;          // the records have been turned into the table: later batches use the atomic kernels
	bool wzero_pending = false;   // the main table is stale (reset without memset): the build overwrites every slot
	WPartGeom wgeom;
	WPartStore wstore = {};       // the kernels' view of `wbuf`
	WPartBufs wbuf;
	// shards and passes of the wide record path (WPartGeom): `wmulti` handles follow the strict protocol
	// begin_pass -> pushes -> [exchange] -> end_pass, ..., finalize; nothing streams through the atomic kernels
	bool wmulti = false;          // sharded and / or several passes
	bool wpass_open = false;      // a pass has been begun and not ended
	bool wplanned = false;        // level-2 tile plan of the current pass made
	uint32_t wnext = 0;           // own-bucket indices [0, wnext) of the current pass have been built
	uint32_t wpasses_done = 0;
	unsigned long long wsaved_totals[2] = {0, 0}; // total_kmers, stored_kmers before a repeated pass over the input
	uint64_t wsaved_reads = 0;
	unsigned long long wsaved_other = 0;          // ... and Counters::other_bytes
	uint64_t wsaved_host_other = 0;
	uint32_t shard_rank = 0;      // shard_index of a sharded handle (any engine)
	bool seed = false;            // SEEDIDX engine: node payload = first occurrence + uniqueness
	// KFREQ engine: counts[4^k] instead of a node table
	bool kfreq = false;
	bool kf_blocks = false;       // KFREQ through the PARTITION engine in its direct-block form (geom.kf == 2, dbgk_partition.h)
	DevBuf<uint8_t> counts;
	uint64_t n_counts = 0;
	uint64_t kf_distinct = 0, kf_sum = 0;
	DevBuf<unsigned long long> kf_bins;    // the 256 device bins of dbgk_kfreq_spectrum, made at its first call
	StageEvent kf_ev[2];
	double kf_spectrum_ms = 0;             // device time of the last k_kf_spectrum

	// PARTITION engine
	bool part = false;            // records are partitioned at push time, table built at finalize
	bool part_built = false;      // finalize already turned the records into the table
	bool part_planned = false;    // level-2 tile plan made for this step (part_plan)
	uint32_t next_bucket = 0;     // own level-1 buckets [0, next_bucket) have been handed to level 2 + build
	uint32_t chunks_used = 0;     // chunk events consumed this step
	uint32_t cursors_used = 0;
	TimedSpan wall_span;
	bool zero_pending = false;    // table content is stale and must be zeroed before a direct-path write
	bool incr = false;            // the table holds nodes of an earlier flush: the next region build loads them back (INCR)
	uint64_t pending_kmers = 0;   // upper bound of the k-mer occurrences sitting in the record store
	uint64_t store_capacity = 0;  // occurrences the record store is sized for (expected_kmers)
	PartGeom geom;
	PartStore store = {};         // the kernels' view of `pbuf`
	PartBufs pbuf;
	uint64_t l2_seen_kmers = 0;      // pending_kmers when the last early level-2 round was launched
	// THREE-LEVEL partition for tables whose level-1 buckets hold 4096 regions (2^33 slots and more): level 2
	// runs as two passes of the same kernel -- MID: every level-1 bucket into fan_mid = n2 / 64 mid buckets (store `mid`,
	// laid out like the level-1 store of a table with r - log2(fan_mid)), FINAL: every mid bucket into its 64 final buckets,
	// written exactly where the two-level form puts them, so the build is the same.  One more pass over the records instead
	// of ~3500 reservation atomics per 8192-record tile.
	bool three = false;
	uint32_t fan_mid = 0;
	PartGeom g_mid, g_fin;
	PartStore s_mid = {}, s_fin = {};
	StageStream stream2;             // finalize: region build of bucket chunk c runs here while level 2 of chunk c+1 runs on `stream`
	std::vector<StageEvent> chunk_ev; // level 2 of chunk c finished
	StageEvent join_ev;
	// sharding: the handle owns slots [geom.slot_lo, geom.slot_hi) of a GLOBAL table of `size` slots
	bool sharded = false;         // shard_count > 1
	bool exchanged = false;       // the caller has filled the inbox (all-to-all) for this step

	// large device-to-host copies (the host KmerSet): slices through pinned buffers, host threads moving them on
	std::vector<PinBuf<char>> d2h_stage;
	std::vector<StageEvent> d2h_ev;
	StageEvent source_read;       // dbgk_push_reads from a pinned caller buffer: the last host-to-device copy out of it
	StageStream copy_stream;      // host-to-device copies of the batches: batch i+1 travels while the kernels of batch i run

	std::vector<TimedSpan> spans, free_spans;
	float phase_ms[PH_COUNT] = {0};
	uint64_t insert_launches = 0;
	uint32_t partition_launches = 0;
	uint32_t uniform_launches = 0;
	// the level-1 forms launched since the last dbgk_reset / dbgk_reset_timings (dbgk_l1_forms_text): the first kL1FormLog of them, and how many there were
	static constexpr uint32_t kL1FormLog = 16;
	L1Form l1_forms[kL1FormLog] = {};
	uint32_t l1_forms_total = 0;

	TableRef tref() const { return TableRef{table, size, magic}; }
	WTable wref() const { return WTable{wnodes, size, magic, wside}; }
};

static int use_device(dbgk_handle *h)
{
	HIPCHK(hipSetDevice(h->device));
	return DBGK_OK;
}

static int span_begin(dbgk_handle *h, int phase, TimedSpan &s, hipStream_t stream = nullptr)
{
	if (!h->free_spans.empty()) {
		s = std::move(h->free_spans.back());
		h->free_spans.pop_back();
	} else {
		if (s.a.create() || s.b.create()) return DBGK_ERR_HIP;
	}
	s.phase = phase;
	HIPCHK(hipEventRecord(s.a, stream ? stream : h->stream));
	return DBGK_OK;
}

static int span_end(dbgk_handle *h, TimedSpan &s, hipStream_t stream = nullptr)
{
	HIPCHK(hipEventRecord(s.b, stream ? stream : h->stream));
	h->spans.push_back(std::move(s));
	return DBGK_OK;
}

// fold finished spans into the per-phase totals.  The caller has synchronised `stream`; region builds
// of a ranged finalize may still be running on `stream2` (their spans are recorded there).
static int collect_spans(dbgk_handle *h)
{
	if (h->stream2) HIPCHK(hipStreamSynchronize(h->stream2));
	for (auto &s : h->spans) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, s.a, s.b));
		h->phase_ms[s.phase] += ms;
		if (s.phase == PH_INSERT) h->insert_launches++;
		if (s.phase == PH_PARTITION) h->partition_launches++;
		h->free_spans.push_back(std::move(s));
	}
	h->spans.clear();
	return DBGK_OK;
}

static inline uint64_t bitmap_words(uint64_t n_bases) { return (n_bases >> 5) + 4; }

// level-1 workgroups per CU: as many as fill the CU's wave slots, unless DBGK_L1_PER_CU says otherwise (experiments with
// 512-thread builds that leave LDS for a workgroup of another kernel)
static int l1_wgs_per_cu()
{
	static const int v = DBGK_EXPERIMENT_ENV("DBGK_L1_PER_CU") ? std::max(1, atoi(DBGK_EXPERIMENT_ENV("DBGK_L1_PER_CU"))) : 1024 / kL1Threads;
	return v;
}

static int grid_for(const dbgk_handle *h, uint64_t items)
{
	uint64_t blocks = (items + kBlock - 1) / kBlock;
	if (blocks < 1) blocks = 1;
	return (int)std::min<uint64_t>(blocks, (uint64_t)h->grid);
}

// ---------------------------------------------------------------------------------------------
// life cycle
// ---------------------------------------------------------------------------------------------
extern "C" int dbgk_abi_version(void) { return DBGK_ABI_VERSION; }

extern "C" int dbgk_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

extern "C" const char *dbgk_last_error(void) { return g_last_error.c_str(); }

extern "C" const char *dbgk_strerror(int status)
{
	switch (status) {
		case DBGK_OK: return "ok";
		case DBGK_ERR_ARG: return "bad argument";
		case DBGK_ERR_HIP: return "HIP runtime error (see dbgk_last_error)";
		case DBGK_ERR_TABLE_FULL: return "k-mer table full";
		case DBGK_ERR_STATE: return "call order violated";
		case DBGK_ERR_NOMEM: return "out of memory";
		case DBGK_ERR_CAPACITY: return "output buffer too small";
		default: return "unknown status";
	}
}

// what dbgk_destroy does behind its null check: every stream of the handle idle with its device current, then the owners free
static void close_handle(dbgk_handle *h)
{
	if (!h) return;
	(void)hipSetDevice(h->device);
	if (h->stream2) (void)hipStreamSynchronize(h->stream2); // region builds of an unfinished ranged finalize
	if (h->stream) (void)hipStreamSynchronize(h->stream);
	if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
	delete h;
}

static int zero_table_now(dbgk_handle *h)
{
	HIPCHK(hipMemsetAsync(h->table, 0, h->tslots * sizeof(Node), h->stream)); // memset_parallel, kmerSet.cpp:358-386
	h->zero_pending = false;
	return DBGK_OK;
}

// empty the record stores of the PARTITION engine (the table and the counters stay)
static int clear_record_store(dbgk_handle *h, bool with_counters = false /* also reset the handle's counters (dbgk_reset) */)
{
	if (h->chunks_used > 0 && h->stream2) { // region builds on the second stream must not race the memsets
		HIPCHK(hipEventRecord(h->join_ev, h->stream2));
		HIPCHK(hipStreamWaitEvent(h->stream, h->join_ev, 0));
	}
	// the heavy-hitter side table is written only once the overflow list is full: zeroed again only then (read BEFORE ovf_n is cleared)
	if (h->store.hh)
		hipLaunchKernelGGL(k_zero_if_greater, dim3(h->n_cu * 4), dim3(kBlock), 0, h->stream, reinterpret_cast<uint4 *>(h->store.hh), h->store.hh_size,
		                   h->store.ovf_n, (unsigned long long)h->store.ovf_cap);
	ZeroList z{};
	int ne = 0;
	auto add = [&](void *q, size_t bytes) { z.p[ne] = q; z.dwords[ne] = (uint32_t)(bytes / 4); ne++; };
	add(h->store.cnt1, (size_t)h->geom.n_ranks * h->geom.B * h->geom.n_sub * 4);
	add(h->store.cnt2, (size_t)h->geom.nb_own * h->geom.n2 * 4);
	if (h->three) add(h->pbuf.cnt_mid, (size_t)h->geom.nb_own * h->fan_mid * 4);
	add(h->store.ovf_n, 16);
	add(h->store.outgoing_n, 8);
	if (h->pbuf.l2_done) add(h->pbuf.l2_done, (size_t)h->geom.n_ranks * h->geom.B * h->geom.n_sub * 8); // done[] and upto[]
	add(h->pbuf.region_cursor, (kMaxBuildLaunches + 2) * sizeof(unsigned int)); // one work cursor per build launch of the next build, + the exact pass's cursor and count
	hipLaunchKernelGGL(k_zero_list, dim3(64), dim3(kBlock), 0, h->stream, z, with_counters ? h->d_ctr : (Counters *)nullptr);
	HIPCHK(hipGetLastError());
	h->part_built = false;
	h->exchanged = false;
	h->part_planned = false;
	h->next_bucket = 0;
	h->chunks_used = 0;
	h->pending_kmers = 0;
	h->l2_seen_kmers = 0;
	return DBGK_OK;
}

// kernels with more than 64 KiB of dynamic LDS have to say so
#define DBGK_LDS_ATTR(KERNEL, BYTES) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BYTES)))

// the host side by engine / concern (one translation unit; the kernels live in dbgk_kernels.h, dbgk_partition.h, dbgk_wide_*.h)
#include "dbgk_host_wide.h"
#include "dbgk_host_partition.h"
#include "dbgk_host_create.h"
#include "dbgk_host_level1.h"
#include "dbgk_host_push.h"
#include "dbgk_host_build.h"
#include "dbgk_host_export.h"
#include "dbgk_host_engines.h"
#include "dbgk_host_misc.h"
#include "dbgk_comm.h"
#include "dbgk_host_wide_links.h"
#include "dbgk_host_emit.h"
#include "dbgk_host_annot.h"
#include "dbgk_host_correct.h"
#include "dbgk_host_spectrum.h"
#include "dbgk_host_map.h"
#include "dbgk_host_clean.h"
#include "dbgk_host_pair.h"
#include "dbgk_host_parse.h"
#include "dbgk_host_format.h"
#include "dbgk_host_maprow.h"
#include "dbgk_host_gz.h"
#include "dbgk_host_inflate.h"
#include "dbgk_host_link.h"
#include "dbgk_host_fill.h"
#include "dbgk_host_super.h"
#include "dbgk_host_contig.h"
#include "dbgk_host_simplify.h"
#include "dbgk_host_align.h"
