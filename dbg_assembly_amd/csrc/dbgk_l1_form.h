// dbgk_l1_form.h -- level 1 of the PARTITION and WIDE record engines: what a kernel form is (L1Form), the one list of
// instantiations per kernel family, and the decision which forms a batch takes (l1_plan).  Plain C++ without HIP: the
// library's host side (dbgk_host_level1.h) builds its launch tables from the lists and launches what the plan says; a
// stand-alone program (tests/l1_form_main.cpp) checks the same lists and the same decision on a machine without a GPU.
#pragma once

#include <cstdint>
#include <cstdio>

namespace dbgk {

// ---------------------------------------------------------------------------------------------
// a kernel form: the template arguments of the level-1 kernels, by name
// ---------------------------------------------------------------------------------------------
enum class L1Family : uint8_t {
	Flat,        // k_extract_scatter: a lane per 16 base positions, read boundaries from the bitmaps
	FlatLin,     // k_extract_scatter_lin: the same with the linear copy-out (many level-1 buckets)
	Uniform,     // k_extract_scatter_uniform: a lane per chunk of valid windows, (nearly) equal-length reads
	Prefix,      // k_extract_scatter_prefix: every read exactly the lanes its windows need
	WideFlat,    // k_wide_scatter_l1
	WideUniform, // k_wide_scatter_l1_uniform
};

struct L1Form {
	L1Family family;
	int wide_d; // how hash / size is computed: 0 = size < 2^31, 1 = size < 2^32, 2 = 64-bit, 3 = KFREQ direct blocks (no hash, no division)
	int c;      // windows per lane (0: the family has a fixed count)
	bool ragged, lin, reg, packed, full, k17; // see k_extract_scatter_uniform; prefix: k17 = its pipelined tile loop
	bool has_dead; // flat families: the batch has trimmed reads (the dead bitmap is read)
	bool pipe;     // wide-uniform: the pipelined tile loop
	int dbg;       // timing experiments (DBGK_EXPERIMENTS builds): 0 in the product

	constexpr bool operator==(const L1Form &o) const
	{
		return family == o.family && wide_d == o.wide_d && c == o.c && ragged == o.ragged && lin == o.lin && reg == o.reg && packed == o.packed &&
		       full == o.full && k17 == o.k17 && has_dead == o.has_dead && pipe == o.pipe && dbg == o.dbg;
	}
};

// One maker per family; the arguments stand in the order of the kernel's template parameters, so a row of the lists
// below reads the same as form and as instantiation.
constexpr L1Form l1_flat(bool has_dead, int dbg, int wide_d) { return {L1Family::Flat, wide_d, 0, false, false, false, false, false, false, has_dead, false, dbg}; }
constexpr L1Form l1_flat_lin(bool has_dead, int wide_d) { return {L1Family::FlatLin, wide_d, 0, false, true, false, false, false, false, has_dead, false, 0}; }
constexpr L1Form l1_uniform(int dbg, int wide_d, int c, bool ragged, bool lin, bool reg, bool packed, bool full, bool k17)
{
	return {L1Family::Uniform, wide_d, c, ragged, lin, reg, packed, full, k17, false, false, dbg};
}
constexpr L1Form l1_prefix(int wide_d, int c, bool k17) { return {L1Family::Prefix, wide_d, c, false, false, false, false, false, k17, false, false, 0}; }
constexpr L1Form l1_wide_flat(bool has_dead, int wide_d) { return {L1Family::WideFlat, wide_d, 0, false, false, false, false, false, false, has_dead, false, 0}; }
constexpr L1Form l1_wide_uniform(int wide_d, bool pipe) { return {L1Family::WideUniform, wide_d, 0, false, false, false, false, false, false, false, pipe, 0}; }

inline const char *l1_family_name(L1Family f)
{
	switch (f) {
	case L1Family::Flat: return "flat";
	case L1Family::FlatLin: return "flat-linear";
	case L1Family::Uniform: return "uniform";
	case L1Family::Prefix: return "prefix";
	case L1Family::WideFlat: return "wide-flat";
	case L1Family::WideUniform: return "wide-uniform";
	}
	return "?";
}

// the form's fields as text (error messages, the stand-alone program's output)
inline void l1_form_text(const L1Form &f, char *buf, size_t n)
{
	snprintf(buf, n, "family=%s wide_d=%d c=%d ragged=%d lin=%d reg=%d packed=%d full=%d k17=%d has_dead=%d pipe=%d dbg=%d", l1_family_name(f.family),
	         f.wide_d, f.c, (int)f.ragged, (int)f.lin, (int)f.reg, (int)f.packed, (int)f.full, (int)f.k17, (int)f.has_dead, (int)f.pipe, f.dbg);
}

// ---------------------------------------------------------------------------------------------
// the instantiations: one list per family, one row per kernel in the library.  X gets the kernel's template arguments.
// The launch tables and the registration of the dynamic LDS sizes are made from these lists and from nothing else.
// ---------------------------------------------------------------------------------------------
#define DBGK_L1_WIDTHS(ROWS, X) ROWS(X, 0) ROWS(X, 1) ROWS(X, 2)

// k_extract_scatter_uniform
//      DBG WIDE_D C  RAGGED LIN    REG    PACKED FULL   K17
#define DBGK_L1_UNIFORM_ROWS_W(X, W)                                                                          \
	X(0, W, 16, false, false, false, false, true, false) /* equal lengths / ragged, k < 17 or KFREQ direct blocks */ \
	X(0, W, 16, true, false, false, false, true, false)                                                       \
	X(0, W, 15, false, false, false, false, true, false)                                                      \
	X(0, W, 15, true, false, false, false, true, false)                                                       \
	X(0, W, 16, false, false, false, false, true, true) /* the pipelined tile loop with 32-bit rolls */       \
	X(0, W, 16, true, false, false, false, true, true)                                                        \
	X(0, W, 15, false, false, false, false, true, true)                                                       \
	X(0, W, 15, true, false, false, false, true, true)                                                        \
	X(0, W, 16, false, false, true, false, true, true) /* regular tiles */                                    \
	X(0, W, 15, false, false, true, false, true, true)                                                        \
	X(0, W, 16, false, false, true, true, true, true)                                                         \
	X(0, W, 15, false, false, true, true, true, true)                                                         \
	X(0, W, 16, false, false, true, false, false, true)                                                       \
	X(0, W, 15, false, false, true, false, false, true)                                                       \
	X(0, W, 16, false, false, true, true, false, true)                                                        \
	X(0, W, 15, false, false, true, true, false, true)                                                        \
	X(0, W, 8, false, true, false, false, true, false) /* the linear form: many level-1 buckets */            \
	X(0, W, 8, true, true, false, false, true, false)                                                         \
	X(0, W, 12, false, true, false, false, true, false)                                                       \
	X(0, W, 12, true, true, false, false, true, false)                                                        \
	X(0, W, 8, false, true, false, false, true, true)                                                         \
	X(0, W, 8, true, true, false, false, true, true)                                                          \
	X(0, W, 12, false, true, false, false, true, true)                                                        \
	X(0, W, 12, true, true, false, false, true, true)
#ifdef DBGK_EXPERIMENTS // timing experiments on cfg2's shape (DBGK_DEBUG_MODE, results are wrong): not in the product library
#define DBGK_L1_UNIFORM_ROWS_DBG(X)                       \
	X(1, 0, 15, false, false, false, false, true, false)  \
	X(2, 0, 15, false, false, false, false, true, false)  \
	X(3, 0, 15, false, false, false, false, true, false)
#define DBGK_L1_FLAT_ROWS_DBG(X) X(false, 1, 0) X(false, 2, 0) X(false, 3, 0)
#else
#define DBGK_L1_UNIFORM_ROWS_DBG(X)
#define DBGK_L1_FLAT_ROWS_DBG(X)
#endif
#define DBGK_L1_UNIFORM_ROWS(X)                                                                                          \
	DBGK_L1_WIDTHS(DBGK_L1_UNIFORM_ROWS_W, X)                                                                            \
	X(0, 3, 15, false, false, false, false, true, false) /* KFREQ, direct blocks: without hash, division, neighbour codes */ \
	X(0, 3, 16, false, false, false, false, true, false)                                                                 \
	DBGK_L1_UNIFORM_ROWS_DBG(X)

// k_extract_scatter_prefix
//      WIDE_D C  K17
#define DBGK_L1_PREFIX_ROWS_W(X, W) X(W, 15, false) X(W, 15, true) X(W, 16, false) X(W, 16, true)
#define DBGK_L1_PREFIX_ROWS(X) DBGK_L1_WIDTHS(DBGK_L1_PREFIX_ROWS_W, X)

// k_extract_scatter
//      HAS_DEAD DBG WIDE_D
#define DBGK_L1_FLAT_ROWS_W(X, W) X(false, 0, W) X(true, 0, W)
#define DBGK_L1_FLAT_ROWS(X) DBGK_L1_WIDTHS(DBGK_L1_FLAT_ROWS_W, X) DBGK_L1_FLAT_ROWS_DBG(X)

// k_extract_scatter_lin and k_wide_scatter_l1
//      HAS_DEAD WIDE_D
#define DBGK_L1_DEAD_ROWS_W(X, W) X(false, W) X(true, W)
#define DBGK_L1_FLAT_LIN_ROWS(X) DBGK_L1_WIDTHS(DBGK_L1_DEAD_ROWS_W, X)
#define DBGK_L1_WIDE_FLAT_ROWS(X) DBGK_L1_WIDTHS(DBGK_L1_DEAD_ROWS_W, X)

// k_wide_scatter_l1_uniform
//      WIDE_D PIPE
#define DBGK_L1_WIDE_UNIFORM_ROWS_W(X, W) X(W, false) X(W, true)
#define DBGK_L1_WIDE_UNIFORM_ROWS(X) DBGK_L1_WIDTHS(DBGK_L1_WIDE_UNIFORM_ROWS_W, X)

// ---------------------------------------------------------------------------------------------
// the decision
// ---------------------------------------------------------------------------------------------
// What the decision needs of the kernels' tile geometry.  The defaults are the product build's; the library fills the
// struct from the kernel headers' own constants (and asserts that an unchanged geometry gives these values).
struct L1Limits {
	uint32_t l1_threads = 1024;          // kL1Threads
	uint32_t pk_words = 1792;            // kPkWords: packed words of a tile's byte range
	uint32_t prefix_max_w = (1u << 22) - 2u; // kPrefixMaxW
	uint32_t prefix_pipe_max_b = 960;    // kPrefixPipeMaxB
	uint32_t wl1_threads = 1024;         // kWL1Threads
	uint32_t wpk_words = 4096;           // kWPkWords
	uint32_t wpipe_pk_words = 912;       // kWPipePkWords

	constexpr bool operator==(const L1Limits &o) const
	{
		return l1_threads == o.l1_threads && pk_words == o.pk_words && prefix_max_w == o.prefix_max_w && prefix_pipe_max_b == o.prefix_pipe_max_b &&
		       wl1_threads == o.wl1_threads && wpk_words == o.wpk_words && wpipe_pk_words == o.wpipe_pk_words;
	}
};

// the facts of a handle and of one batch, gathered once per batch
struct L1Facts {
	L1Limits lim;
	// the handle
	bool part = false, seed = false, kfreq = false, wide = false;
	bool wrec = false;          // WIDE handle that is still collecting records
	int kmer_size = 0;
	uint64_t max_read_len = 0;
	uint32_t n1 = 0, kf = 0;    // PartGeom: level-1 buckets; kf == 2: KFREQ with direct blocks
	uint64_t geom_size = 0;     // PartGeom::size
	uint64_t size = 0;          // the handle's hash modulus (the WIDE engine divides by this one)
	// the batch
	uint64_t n_reads = 0, n_bases = 0;
	int has_long = 0;           // some read is longer than maxReadLen (trimmed)
	int64_t uniform_len = 0;    // every read this long; 0 = lengths differ
	uint64_t len_max = 0;       // longest read
	bool packed = false;        // 2-bit codes instead of ASCII
	// test hooks (DBGK_TEST_HOOKS), read once per batch: the tests switch them between handles
	int l1_linear = -1, l1_prefix = -1; // -1: not set
	bool l1_plain = false, wide_l1_plain = false;
	// experiments (DBGK_EXPERIMENTS builds; all unset in the product)
	bool l1_flat = false;       // DBGK_L1_FLAT: the general kernel everywhere
	bool dbg_set = false;       // DBGK_DEBUG_MODE is set,
	int dbg_mode = 0;           // and its value
	bool no_reg = false;        // DBGK_L1_NO_REG: A/B, the general form instead of regular tiles
	int lin_c = 0;              // DBGK_L1_LINEAR_C: 12 or 8 windows per lane of the linear form (0: not set)
};

// UniformGeom and WUniformGeom (which is the first five fields) as the decision fills them
struct L1Geom {
	uint32_t L = 0, W = 0, Q = 0, qmagic = 0;
	uint64_t n_lanes = 0;
	uint32_t lq = 0, tile_blocks = 0;
};

struct L1Launch {
	L1Form form;
	L1Geom geom;             // uniform families
	uint64_t first_read = 0; // the launch covers n_reads reads from this one
	uint64_t n_reads = 0;
	uint64_t tiles = 0;      // workgroup tiles of work: the grid is this many, capped by what the device holds at once (0: the cap itself)
};

struct L1Plan {
	int umode = 0;       // 0 = no uniform form, 1 = equal lengths, 2 = ragged
	bool prefix = false; // the prefix form (umode then says what it replaced)
	int n = 0;           // launches: two = regular tiles, then the rest
	L1Launch launch[2];
};

// how hash / size is computed for a table of `size` slots (direct blocks: the 64-bit slot path)
inline int l1_width(uint64_t size, bool direct_blocks = false) { return (direct_blocks || size >= (1ull << 32)) ? 2 : (size >= (1ull << 31) ? 1 : 0); }

// 16 or 15 windows per lane, whichever leaves fewer empty slots at the end of a full-length read (W = 120: 15 -> none)
inline uint32_t l1_windows_per_lane(uint32_t W) { return (W + 14u) / 15u * 15u - W < (W + 15u) / 16u * 16u - W ? 15u : 16u; }
// the linear form: 12 or 8 windows per lane, whichever leaves fewer empty slots at the end of a read (W = 120: both none -> 12)
inline uint32_t l1_lin_windows_per_lane(uint32_t W) { return (W + 11u) / 12u * 12u - W <= (W + 7u) / 8u * 8u - W ? 12u : 8u; }

// Many level-1 buckets (big tables; every rank of a multi-GPU job partitions by the GLOBAL table's buckets) take the linear
// forms.  Measured on cfg2's reads, level 1 in ms, wave-per-bucket / linear with 8 / with 12 windows:
// n1 = 143: 5.57 / 6.76 / 6.05, 573: 8.13 / 7.57 / 6.81, 1023: 10.61 / 7.76 / 6.99 (287: 6.34 / 6.77 / -).
// (round 5, both forms pipelined, profiles/r05_l1_forms_by_buckets.txt, wave-per-bucket / linear with 12 windows: n1 = 144: 4.34 / 5.08,
// 287: 4.80 / 5.26, 573: 6.83 / 5.87, 1023: 12.27 / 6.11 -- the lines cross near 330)
// The hook l1_linear=0/1 forces the choice.
constexpr uint32_t kL1LinearAboveN1 = 320;
inline bool l1_takes_linear(uint32_t n1, int hook) { return hook == 1 || (hook < 0 && n1 > kL1LinearAboveN1); }

// The lane-per-chunk-of-valid-windows level-1 kernel (k_extract_scatter_uniform) applies when nothing is
// trimmed (longest read <= maxReadLen), the longest read has at least 64 windows (a tile's byte range
// must fit its LDS image) and either
//   * every read has that length and they lie back to back from offset 0 (EQUAL), or
//   * lengths differ, but giving every read the lane count of the longest one still needs fewer lane
//     slots than the flat kernel has positions (RAGGED: reads mostly full length, some shorter).
// Returns 0 = flat kernel, 1 = equal, 2 = ragged; fills U and c (windows per lane).
// lin (out): the linear level-1 form (c = 12 or 8, linear copy-out) is to be used -- many level-1 buckets
inline int uniform_mode(const L1Facts &f, L1Geom &U, uint32_t &c, bool &lin)
{
	lin = false;
	const uint64_t n_reads = f.n_reads, threads = f.lim.l1_threads;
	if (f.l1_flat || f.has_long || n_reads == 0) return 0;
	if (f.dbg_mode && (f.uniform_len != 150 || f.kmer_size != 31 || f.geom_size >= (1ull << 31))) return 0; // debug builds: cfg2's shape only
	const uint64_t L = f.uniform_len > 0 ? (uint64_t)f.uniform_len : f.len_max, k = (uint64_t)f.kmer_size;
	if (L > f.max_read_len || L < k + 63 || L >= (1ull << 24)) return 0;
	const uint32_t W = (uint32_t)(L - k + 1);
	c = l1_windows_per_lane(W);
	const uint64_t C = c, Q = (W + C - 1) / C;
	if (Q >= 2048 || n_reads * Q >= (1ull << 32)) return 0;
	if ((threads / Q + 2) * L + 96 > (uint64_t)f.lim.pk_words * 16) return 0; // bytes a tile of kL1Threads lanes can touch
	U.L = (uint32_t)L;
	U.W = W;
	U.Q = (uint32_t)Q;
	U.qmagic = ((1u << 22) + U.Q - 1u) / U.Q;
	U.n_lanes = n_reads * Q;
	U.lq = 0;
	U.tile_blocks = 0; // 0: no regular tiles
	// (the regular form also assumes k >= 17 -- the rolls then only touch the high words -- and a graph handle: no KFREQ neighbour
	// codes; reads that fill their lanes exactly, Q C == W, take its FULL instantiation, the others test every position's validity)
	if ((Q & (Q - 1)) == 0 && Q <= threads && ((threads / Q) * L) % 16 == 0 && (threads / Q) * L / 16 + 8 <= (uint64_t)f.lim.pk_words && k >= 17 &&
	    !f.kfreq) {
		while ((1ull << U.lq) < Q) U.lq++;
		U.tile_blocks = (uint32_t)((threads / Q) * L / 16);
	}
	int mode;
	if (f.uniform_len > 0) mode = f.n_bases == n_reads * L ? 1 : 0;
	else mode = (double)(n_reads * Q * C) <= 0.93 * (double)f.n_bases ? 2 : 0; // mostly full-length reads: the ragged form
	if (mode == 0) return 0;
	uint32_t cl = l1_lin_windows_per_lane(W);
	if (f.lin_c) cl = (uint32_t)f.lin_c; // measurements
	const uint64_t CL = cl, QL = (W + CL - 1) / CL;
	bool fits = QL < 2048 && n_reads * QL < (1ull << 32) && (threads / QL + 2) * L + 96 <= (uint64_t)f.lim.pk_words * 16;
	if (mode == 2) fits = fits && (double)(n_reads * QL * CL) <= 0.93 * (double)f.n_bases;
	if (fits && l1_takes_linear(f.n1, f.l1_linear)) {
		lin = true;
		c = cl;
		U.tile_blocks = 0;
		U.Q = (uint32_t)QL;
		U.qmagic = ((1u << 22) + U.Q - 1u) / U.Q;
		U.n_lanes = n_reads * QL;
	}
	return mode;
}

// WIDE record path: can this batch take the equal-length level-1 kernel (k_wide_scatter_l1_uniform)?
inline int wide_uniform_mode(const L1Facts &f, L1Geom &U)
{
	const uint64_t n_reads = f.n_reads, threads = f.lim.wl1_threads;
	if (f.l1_flat || f.has_long || n_reads == 0 || f.uniform_len <= 0) return 0;
	const uint64_t L = (uint64_t)f.uniform_len, k = (uint64_t)f.kmer_size;
	if (L > f.max_read_len || L < k || L >= (1ull << 24) || f.n_bases != n_reads * L) return 0;
	const uint32_t W = (uint32_t)(L - k + 1);
	const uint64_t Q = (W + 7u) / 8u;
	if (Q >= 2048 || n_reads * Q >= (1ull << 40)) return 0;
	if ((threads / Q + 2) * L + 96 > (uint64_t)(f.lim.wpk_words - 8u) * 16) return 0; // bytes a tile of 1024 lanes can touch
	if ((double)(n_reads * Q * 8) > 0.93 * (double)f.n_bases) return 0; // (k small against L: the flat kernel wastes little)
	U.L = (uint32_t)L;
	U.W = W;
	U.Q = (uint32_t)Q;
	U.qmagic = ((1u << 22) + U.Q - 1u) / U.Q;
	U.n_lanes = n_reads * Q;
	return 1;
}

// The PREFIX form of level 1 (k_extract_scatter_prefix: every read exactly the lanes its windows need, reads of any lengths,
// trimmed ones included) takes what would otherwise go through the flat kernel -- a fifth of whose positions straddle a
// read boundary at 150 bases and k = 31 -- and the batches of the ragged form as well; not with many level-1 buckets (the
// linear forms), not for reads of more than 4 M windows.  The hook l1_prefix=0 switches it off (ragged / flat as before).
inline bool prefix_wanted(const L1Facts &f, int umode)
{
	if (!f.part || f.seed || f.wrec || f.l1_flat || f.dbg_set || f.l1_prefix == 0) return false;
	if (l1_takes_linear(f.n1, f.l1_linear)) return false;
	if (f.len_max > (uint64_t)f.lim.prefix_max_w || f.n_bases / 15 + f.n_reads >= (1ull << 32)) return false;
	return umode == 0 || umode == 2; // (measured on cfg2t, level 1 per step: prefix 5.32 ms, ragged 5.72, flat 6.05 + 0.14 of bitmaps: profiles/r04_cfg2t_level1_forms_ab.json)
}

// The level-1 launches of one batch of a PARTITION handle (not SEEDIDX) or of a WIDE handle that collects records.
inline L1Plan l1_plan(const L1Facts &f)
{
	L1Plan plan{};
	auto add = [&](const L1Form &form, const L1Geom &g, uint64_t first_read, uint64_t n_reads, uint64_t tiles) {
		plan.launch[plan.n++] = L1Launch{form, g, first_read, n_reads, tiles};
	};
	auto tiles_of = [](uint64_t items, uint64_t threads) { return (items + threads - 1) / threads; };
	const uint64_t n_chunks = (f.n_bases + 15) >> 4; // the flat families: a lane per 16 positions
	L1Geom U;
	if (f.wrec) {
		plan.umode = wide_uniform_mode(f, U);
		const int wd = l1_width(f.size);
		if (plan.umode > 0) {
			// the pipelined form keeps a tile's packed words beside the stage buffer: taken when the bytes a tile of 1024 lanes can touch fit there
			const bool pipe = !f.wide_l1_plain && ((uint64_t)f.lim.wl1_threads / U.Q + 2) * U.L + 96 <= (uint64_t)(f.lim.wpipe_pk_words - 8u) * 16;
			add(l1_wide_uniform(wd, pipe), U, 0, f.n_reads, tiles_of(U.n_lanes, f.lim.wl1_threads));
		} else
			add(l1_wide_flat(f.has_long != 0, wd), U, 0, f.n_reads, tiles_of(n_chunks, f.lim.wl1_threads));
		return plan;
	}
	uint32_t c = 16;
	bool lin = false;
	plan.umode = uniform_mode(f, U, c, lin);
	plan.prefix = prefix_wanted(f, plan.umode);
	const int wide = l1_width(f.geom_size, f.kf == 2u);
	if (plan.prefix) {
		const uint64_t len = f.len_max < f.max_read_len ? f.len_max : f.max_read_len; // (longer reads are trimmed)
		const uint32_t W_max = len >= (uint64_t)f.kmer_size ? (uint32_t)len - (uint32_t)f.kmer_size + 1u : 1u;
		const bool pipe = f.kmer_size >= 17 && f.kf != 2u && f.n1 <= f.lim.prefix_pipe_max_b && !f.l1_plain; // the pipelined tile loop
		add(l1_prefix(wide, (int)l1_windows_per_lane(W_max), pipe), L1Geom{}, 0, f.n_reads, 0);
	} else if (plan.umode > 0) {
		const bool ragged = plan.umode == 2;
		// equal lengths, ragged: the pipelined tile loop (32-bit rolls; 64-bit records -- a KFREQ handle with direct blocks has its own instantiation)
		const bool k17 = f.kmer_size >= 17 && f.kf != 2u && !f.l1_plain;
		uint64_t done_reads = 0;
		if (!f.dbg_mode && !f.no_reg && !f.l1_plain && plan.umode == 1 && !lin && U.tile_blocks) {
			// regular tiles: kL1Threads / Q whole reads each, from a 16-byte boundary; the reads behind the last whole tile
			// (fewer than kL1Threads / Q) go through the general form below
			const uint64_t reads_per_tile = (uint64_t)f.lim.l1_threads / U.Q, full_tiles = f.n_reads / reads_per_tile;
			if (full_tiles) {
				L1Geom UR = U;
				UR.n_lanes = full_tiles * f.lim.l1_threads;
				const bool full = (uint64_t)U.Q * c == (uint64_t)U.W; // the reads fill their lanes exactly
				done_reads = full_tiles * reads_per_tile;
				add(l1_uniform(0, wide, (int)c, false, false, true, f.packed, full, true), UR, 0, done_reads, full_tiles);
				U.n_lanes = (f.n_reads - done_reads) * U.Q;
			}
		}
		if (U.n_lanes) {
			L1Form form = l1_uniform(0, wide, (int)c, ragged, lin, false, false, true, k17);
			if (f.dbg_mode >= 1 && f.dbg_mode <= 3) // timing experiments on cfg2's shape (C = 15, equal lengths, size < 2^31): results are wrong
				form = l1_uniform(f.dbg_mode, 0, 15, false, false, false, false, true, false);
			else if (!lin && f.kf == 2u && !ragged) // KFREQ, direct blocks: the instantiation without hash, division and neighbour codes
				form = l1_uniform(0, 3, (int)c, false, false, false, false, true, false);
			add(form, U, done_reads, f.n_reads - done_reads, tiles_of(U.n_lanes, f.lim.l1_threads));
		}
	} else {
		const uint64_t tiles = tiles_of(n_chunks, f.lim.l1_threads);
		const bool dead = f.has_long != 0;
		if (!f.dbg_mode && l1_takes_linear(f.n1, f.l1_linear)) add(l1_flat_lin(dead, wide), U, 0, f.n_reads, tiles); // many level-1 buckets: the linear form
		else if (wide == 0 && f.dbg_mode >= 1 && f.dbg_mode <= 3) add(l1_flat(false, f.dbg_mode, 0), U, 0, f.n_reads, tiles);
		else add(l1_flat(dead, 0, wide), U, 0, f.n_reads, tiles);
	}
	return plan;
}

} // namespace dbgk
