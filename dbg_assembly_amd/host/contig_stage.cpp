// contig_stage.cpp -- the contig stage of debruijn_contig (see contig_stage.h).
//
// The three simplification passes decide on the host in list order: each removal re-derives the links of the nodes at its ends
// (recalculate_kmer_links, DBG_contig/contig.cpp:210-277) and so changes what later list entries see.  That holds for the decisions,
// not for the walks: a removal sets the delete flag of its path's nodes and recalculates one or two end nodes, and a later walk
// differs only if it touches one of those slots.  So before a pass all of its walks (get_linear_path, :779-827) are traced at once on
// the GPU against the table as it stands then (SIMPLIFY section of include/dbgk.h), the loops consume the traces in list order, and
// a bitmap of the slots changed since says where a trace no longer holds: there the host walks the path itself, as it did for every
// path before (traced_or_walked).  After a pass the changed slots go to the device copy, which the read-out then uses as it is.
// The read-out runs on the GPU through the CONTIG section of include/dbgk.h; header strings, the sort by length, ids and the -M split
// are done here.  Test hook simplify_host=1: no tracing, every path walked on the host.
// The bubbles pass aligns two arms where their lengths differ or too many of their bases do (global_aligning).  An alignment is a function
// of its two strings, so those of all bubbles the pass's traces show are computed at once on the GPU when the pass begins
// (collect_alignments, dbgk_align_pairs); the ordered loop takes a result if and only if the strings it holds at that moment are byte
// for byte the submitted ones, and aligns on the host otherwise.  Test hooks: align_host=1, nothing is submitted; align_stale=1, see collect_alignments.
// Line numbers name DBG_contig/contig.cpp unless another file is given.
//
// The stage is written once over the key type (Stage<G>): Keys64 is `kset` with the reference's uint64_t k-mers, Keys128 is
// `kset_wide` with 128-bit k-mers (k = 33..63; PARITY UNPINNED above k = 32: the reference stops at 31, the rules are those of
// include/dbgk_wide.h and kmerSet.h's hash_code128, each of which is the 64-bit rule when the high word is 0).  Needleman-Wunsch,
// the sort, the ids and the -M split never see a key.
#include "contig_stage.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "DBGgraph.h"
#include "dbgk.h"
#include "dbgk_env.h"
#include "dbgk_wide.h"

// the command line's options (defined in main.cpp)
extern int KmerFreqCutoff, is_remove_tip, Tip_len_cutoff, is_remove_lowedge, LowCovEdge_len_cutoff, is_remove_bubble, Bubble_len_cutoff,
    Contig_len_cutoff;
extern double Tip_depth_cutoff, LowCovEdge_depth_cutoff, Bubble_len_diff_rate_cutoff, Bubble_base_diff_rate_cutoff;

namespace {

// the 2-byte link record of every slot, laid out as dbgk_export_host_table_links writes it (contig.h:31-42): l_link_num |
// l_link_base << 2 | r_link_num << 4 | r_link_base << 6, bit 8 linear, bits 9..12 in_tip, in_bubble, in_lowedge, in_repeat
uint16_t *klink = NULL;
const uint32_t kClearBase[4] = {0x00FFFFFFu, 0xFF00FFFFu, 0xFFFF00FFu, 0xFFFFFF00u};   // BitMaskVal, :31
enum { IN_TIP = 1 << 9, IN_BUBBLE = 1 << 10, IN_LOWEDGE = 1 << 11, IN_REPEAT = 1 << 12 };

inline int l_num(uint64_t i) { return klink[i] & 3; }
inline int l_base(uint64_t i) { return (klink[i] >> 2) & 3; }
inline int r_num(uint64_t i) { return (klink[i] >> 4) & 3; }
inline int r_base(uint64_t i) { return (klink[i] >> 6) & 3; }

double ms_since(const std::chrono::steady_clock::time_point &t0)
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the table of 16-byte nodes, 64-bit k-mers: the reference's
struct Keys64 {
	typedef uint64_t Key;
	static uint64_t size() { return kset->size; }
	static uint8_t *nul_flag() { return kset->nul_flag; }
	static uint8_t *del_flag() { return kset->del_flag; }
	static Key kmer(uint64_t i) { return kset->array[i].kmer; }
	static uint32_t &l_link(uint64_t i) { return kset->array[i].l_link; }
	static uint32_t &r_link(uint64_t i) { return kset->array[i].r_link; }
	static uint64_t exist(Key key) { return exist_kmerset(kset, key); }
	static Key next_leftward(Key kmer, int base) { return (kmer >> 2) + ((uint64_t)base << ((KmerSize - 1) * 2)); }   // contig.h:119-123
	static Key next_rightward(Key kmer, int base) { return ((kmer << 2) | (uint64_t)base) & KmerHeadMaskVal; }        // contig.h:127-130
	static Key rev_com(Key kmer) { return get_rev_com_kbit(kmer, KmerSize); }
	static std::string text(Key kmer) { return bit2seq(kmer, KmerSize); }
	static std::string decimal(Key kmer) { return std::to_string(kmer); }
	static int create(const dbgk_contig_params *p, int device, dbgk_contig **h) { return dbgk_contig_create(p, device, h); }
	static int set_table(dbgk_contig *h)
	{
		return dbgk_contig_set_table(h, kset->size, reinterpret_cast<const dbgk_node *>(kset->array), kset->nul_flag, kset->del_flag, klink);
	}
};

// the table of 32-byte nodes, 128-bit k-mers {kmer_hi, kmer_lo}
struct Keys128 {
	typedef unsigned __int128 Key;
	static Key make(uint64_t hi, uint64_t lo) { return ((Key)hi << 64) | lo; }
	static uint64_t size() { return kset_wide->size; }
	static uint8_t *nul_flag() { return kset_wide->nul_flag; }
	static uint8_t *del_flag() { return kset_wide->del_flag; }
	static Key kmer(uint64_t i) { return make(kset_wide->array[i].kmer_hi, kset_wide->array[i].kmer_lo); }
	static uint32_t &l_link(uint64_t i) { return kset_wide->array[i].l_link; }
	static uint32_t &r_link(uint64_t i) { return kset_wide->array[i].r_link; }
	static uint64_t exist(Key key) { return exist_kmerset128(kset_wide, (uint64_t)(key >> 64), (uint64_t)key); }
	// the base lands at bit 2 (k - 1): in the high word from k = 33 on; two bits move down from the high word
	static Key next_leftward(Key kmer, int base) { return (kmer >> 2) + ((Key)base << ((KmerSize - 1) * 2)); }
	// two bits move up into the high word; 2 k <= 126 bits stay
	static Key next_rightward(Key kmer, int base) { return ((kmer << 2) | (Key)base) & ((((Key)1) << (2 * KmerSize)) - 1); }
	static Key rev_com(Key kmer)
	{
		const dbgk_wide::Key128 r = dbgk_wide::revcomp(dbgk_wide::Key128{(uint64_t)(kmer >> 64), (uint64_t)kmer}, KmerSize);
		return make(r.hi, r.lo);
	}
	static std::string text(Key kmer)
	{
		std::string s(KmerSize, 'A');
		for (int j = 0; j < KmerSize; j++) s[j] = bases[(int)(kmer >> (2 * (KmerSize - 1 - j))) & 3];
		return s;
	}
	static std::string decimal(Key kmer)   // with a high word of 0 the reference's text
	{
		if (!kmer) return "0";
		std::string s;
		for (; kmer; kmer /= 10) s.push_back((char)('0' + (int)(kmer % 10)));
		std::reverse(s.begin(), s.end());
		return s;
	}
	static int create(const dbgk_contig_params *p, int device, dbgk_contig **h) { return dbgk_wide_contig_create(p, device, h); }
	static int set_table(dbgk_contig *h)
	{
		return dbgk_wide_contig_set_table(h, kset_wide->size, reinterpret_cast<const dbgk_node32 *>(kset_wide->array), kset_wide->nul_flag,
		                                  kset_wide->del_flag, klink);
	}
};

// compare_two_seq_simple, :587-595: gap columns do not count
int count_differences(const std::string &a, const std::string &b)
{
	int n = 0;
	for (size_t i = 0; i < a.size(); i++)
		if (a[i] != b[i] && a[i] != '-' && b[i] != '-') n++;
	return n;
}

// global_aligning, global_aligning.cpp:98-182: Needleman-Wunsch with match 3, mismatch -5, gap -5; on equal scores a
// substitution goes before a gap in the first sequence, that before a gap in the second (get_max_score, :20-35)
void global_align(const std::string &si, const std::string &sj, std::string &ai, std::string &aj)
{
	const int gap = -5, ni = si.size(), nj = sj.size(), w = nj + 1;
	std::vector<int> score((size_t)(ni + 1) * w), from((size_t)(ni + 1) * w);
	score[0] = from[0] = 0;
	for (int j = 1; j <= nj; j++) score[j] = gap * j, from[j] = 1;
	for (int i = 1; i <= ni; i++) score[i * w] = gap * i, from[i * w] = 2;
	for (int i = 1; i <= ni; i++)
		for (int j = 1; j <= nj; j++) {
			const char a = si[i - 1], b = sj[j - 1];   // A C G T only: paths are written from 2-bit codes
			const int sub = score[(i - 1) * w + j - 1] + (a == b ? 3 : -5), gi = score[i * w + j - 1] + gap, gj = score[(i - 1) * w + j] + gap;
			int best, dir;
			if (sub >= gi && sub >= gj) best = sub, dir = 0;
			else if (gi > sub && gi >= gj) best = gi, dir = 1;
			else best = gj, dir = 2;
			score[i * w + j] = best;
			from[i * w + j] = dir;
		}
	int i = ni, j = nj;
	do {                             // trace_back, global_aligning.cpp:39-68
		const int dir = from[i * w + j];
		if (dir == 0) ai.push_back(si[--i]), aj.push_back(sj[--j]);
		else if (dir == 1) ai.push_back('-'), aj.push_back(sj[--j]);
		else ai.push_back(si[--i]), aj.push_back('-');
	} while (i > 0 || j > 0);
	std::reverse(ai.begin(), ai.end());
	std::reverse(aj.begin(), aj.end());
}

// get_branch_bases, :361-370
void branch_bases(uint32_t link, std::vector<uint8_t> &vb, std::vector<uint8_t> &vd)
{
	for (int j = 0; j < 4; j++) {
		const int depth = get_next_kmer_depth(link, j);
		if (depth > KmerFreqCutoff) {
			vb.push_back(j);
			vd.push_back(depth);
		}
	}
}

void finished(const char *word)
{
	time_end = clock();
	cerr << word << " Run time: " << double(time_end - time_start) / CLOCKS_PER_SEC << endl;
}

struct Path {                      // what get_linear_path returns
	int len = 0, depth = 0;
	std::vector<uint64_t> nodes;
	std::string str;
	uint64_t last = 0;
	const char *mark = "linear";
};

template <class G>
struct Stage {
typedef typename G::Key Key;

// "no such node" is slot size(); the reference looks at klink[G::size()] there (:810, :648), this build calls it not linear
static bool is_linear(uint64_t i) { return i != G::size() && (klink[i] & 0x100); }
// bits 9..12 are read by no walk: the slot goes to the device copy, but no trace is lost over it
static void set_flag(uint64_t i, int flag)
{
	if (i == G::size()) return;
	klink[i] |= flag;
	if (handle) dirty.push_back(i);
}

// ---- the traced walks of the pass that is running ----
static dbgk_contig *handle;                    // made before the first enabled pass, kept through the read-out
static bool have_traces;                       // this pass has traces (its cutoff fits DBGK_TRACE_MAX_CUTOFF)
static std::vector<dbgk_trace_row> rows;
static std::vector<uint64_t> node_first;
static std::vector<uint32_t> trace_nodes;
static std::vector<uint8_t> trace_bases;
static std::vector<uint8_t> changed;           // one bit per slot: changed since the traces were taken
static std::vector<uint64_t> dirty;            // slots to carry to the device copy after the pass
static uint64_t n_used, n_fell_back;

// ---- the alignments of the bubbles pass, computed when it begins ----
static std::vector<int64_t> pair_of;           // per entry of the pass's list: the pair it submitted, or -1
static std::vector<std::string> submitted;     // pair p: strings 2 p and 2 p + 1, as composed from the traces
static std::vector<dbgk_align_row> align_rows;
static std::vector<uint64_t> align_first;
static std::string align_i, align_j;
static uint64_t n_candidates, n_too_long, n_align_used, n_align_host;

static bool is_changed(uint64_t i) { return (changed[i >> 3] >> (i & 7)) & 1; }
static void mark_changed(uint64_t i)
{
	if (!handle) return;
	changed[i >> 3] |= (uint8_t)(1u << (i & 7));
	dirty.push_back(i);
}

static int gpu_failed(int rc)
{
	cerr << "tracing the simplification paths on the GPU failed: " << dbgk_strerror(rc) << " " << dbgk_last_error() << endl;
	return rc;
}

// the handle with the table as it stands; 0, or a DBGK_ERR_* code
static int open_handle()
{
	dbgk_contig_params prm = {KmerSize, KmerFreqCutoff < 0 ? 0 : KmerFreqCutoff, Contig_len_cutoff, 0};
	const char *dev = getenv("DBGK_DEVICE");
	int rc = G::create(&prm, dev ? atoi(dev) : 0, &handle);
	if (!rc) rc = G::set_table(handle);
	if (rc && handle) {
		dbgk_contig_destroy(handle);
		handle = NULL;
	}
	return rc;
}

// Before a pass: trace its walks -- `list` holds tips (requests (idx, l_num(idx) == 1 ? -1 : +1)) or branching nodes (8 rows each).
// get_branch_bases compares with KmerFreqCutoff as it is; the handle holds max(KmerFreqCutoff, 0).  For a negative cutoff the two differ
// on edges of depth 0: the host admits them (0 > -1), the kernel's row says BELOW_CUTOFF.  Such a row has no trace, so the host walks
// that path itself and the result is the same
static int begin_pass(const std::vector<uint64_t> &list, bool tips, int len_cutoff)
{
	have_traces = false;
	n_used = n_fell_back = 0;
	if (dbgk_hook("simplify_host")) return 0;
	if (!handle) {
		const int rc = open_handle();
		if (rc) return gpu_failed(rc);
	}
	changed.assign(G::size() / 8 + 1, 0);
	dirty.clear();
	if (len_cutoff > DBGK_TRACE_MAX_CUTOFF) return 0;
	dbgk_trace_summary sum;
	int rc;
	if (tips) {
		std::vector<dbgk_trace_request> req(list.size());
		for (size_t i = 0; i < list.size(); i++) req[i] = dbgk_trace_request{list[i], l_num(list[i]) == 1 ? -1 : 1, 0};
		rc = dbgk_simplify_trace(handle, req.data(), req.size(), len_cutoff, &sum);
	} else {
		rc = dbgk_simplify_trace_branches(handle, list.data(), list.size(), len_cutoff, &sum);
	}
	if (rc) return gpu_failed(rc);
	rows.resize(sum.rows);
	node_first.resize(sum.rows + 1);
	trace_nodes.resize(sum.nodes);
	trace_bases.resize(sum.nodes);
	rc = dbgk_simplify_trace_results(handle, rows.data(), node_first.data(), trace_nodes.data(), trace_bases.data());
	if (rc) return gpu_failed(rc);
	have_traces = true;
	return 0;
}

// the string of a traced row, as path_sequence gives it for the walk
static std::string traced_sequence(uint64_t row)
{
	const dbgk_trace_row &r = rows[row];
	std::string steps(r.len, 'A');
	for (uint32_t j = 0; j < r.len; j++) steps[j] = bases[trace_bases[node_first[row] + j]];
	return path_sequence(r.start, r.direct, steps);
}

// Before the bubbles pass, behind begin_pass: every list entry that is a bubble in the pass's traces -- two edges on one side, one on the
// other, both arms traced, both ending on the same node -- has its two strings composed as remove_bubbles composes them, and those that
// remove_bubbles would align (the same expressions, in double) go to the GPU in one call.  Reads rows, never traced_or_walked: the pass's
// counts of used traces are not touched.  Without traces, or under the test hook align_host, nothing is submitted.
static int collect_alignments(const std::vector<uint64_t> &branches)
{
	pair_of.clear();
	submitted.clear();
	align_rows.clear();
	n_candidates = n_too_long = n_align_used = n_align_host = 0;
	if (!have_traces) return 0;
	const bool submit = !dbgk_hook("align_host");
	// test hook align_stale: every pair goes up with its two strings exchanged, so no result is the one the loop asks for -- the only way
	// to the other side of the comparison in aligned_arms, which no removal of this pass can bring about
	const bool exchange = dbgk_hook("align_stale") != NULL;
	pair_of.assign(branches.size(), -1);
	for (size_t i = 0; i < branches.size(); i++) {
		const uint64_t idx = branches[i];
		int direct = 0;
		std::vector<uint8_t> vb, vd;
		if (l_num(idx) == 2 && r_num(idx) == 1) {
			direct = -1;
			branch_bases(G::l_link(idx), vb, vd);
		} else if (l_num(idx) == 1 && r_num(idx) == 2) {
			direct = 1;
			branch_bases(G::r_link(idx), vb, vd);
		} else {
			continue;
		}
		if (vb.size() < 2) continue;
		const uint64_t row1 = 8 * i + (direct == 1 ? 0 : 4) + vb[0], row2 = 8 * i + (direct == 1 ? 0 : 4) + vb[1];
		const dbgk_trace_row &r1 = rows[row1], &r2 = rows[row2];
		if (r1.status != DBGK_TRACE_TRACED || r2.status != DBGK_TRACE_TRACED || r1.last != r2.last) continue;
		n_candidates++;
		std::string s1 = traced_sequence(row1), s2 = traced_sequence(row2);
		if (r1.direct != r2.direct) {
			std::reverse(s1.begin(), s1.end());
			complement_sequence(s1);
		}
		const int len1 = (int)r1.len + 1, len2 = (int)r2.len + 1;
		double diff_rate = 0;
		if (len1 == len2) diff_rate = (double)count_differences(s1, s2) / len1;
		if (!(len1 != len2 || diff_rate > Bubble_base_diff_rate_cutoff) || !submit) continue;
		if (exchange) s1.swap(s2);
		pair_of[i] = (int64_t)(submitted.size() / 2);
		submitted.push_back(s1);
		submitted.push_back(s2);
	}
	if (submitted.empty()) return 0;
	std::string seqs;
	std::vector<uint64_t> offsets(1, 0);
	for (const std::string &t : submitted) {
		seqs += t;
		offsets.push_back(seqs.size());
	}
	dbgk_align_summary sum;
	int rc = dbgk_align_pairs(handle, seqs.data(), offsets.data(), submitted.size() / 2, &sum);
	if (rc) return gpu_failed(rc);
	align_rows.resize(sum.pairs);
	align_first.resize(sum.pairs + 1);
	align_i.assign(sum.aligned_bytes, '\0');
	align_j.assign(sum.aligned_bytes, '\0');
	rc = dbgk_align_results(handle, align_rows.data(), align_first.data(), &align_i[0], &align_j[0]);
	if (rc) return gpu_failed(rc);
	n_too_long = sum.too_long;
	return 0;
}

// global_aligning(s1, s2) for entry i of the pass's list: the GPU's strings if and only if this entry submitted a pair, the strings the
// loop holds now are byte for byte the submitted ones, and the pair was aligned; on the host otherwise
static void aligned_arms(size_t i, const std::string &s1, const std::string &s2, std::string &a1, std::string &a2)
{
	if (i < pair_of.size() && pair_of[i] >= 0) {
		const uint64_t p = (uint64_t)pair_of[i];
		if (align_rows[p].status == DBGK_ALIGN_DONE && submitted[2 * p] == s1 && submitted[2 * p + 1] == s2) {
			a1.assign(align_i, align_first[p], align_first[p + 1] - align_first[p]);
			a2.assign(align_j, align_first[p], align_first[p + 1] - align_first[p]);
			n_align_used++;
			return;
		}
	}
	global_align(s1, s2, a1, a2);
	n_align_host++;
}

// the line of the bubbles pass's alignments under DBGK_TIMINGS
static void report_alignments(dbgk_align_timing &before)
{
	if (!handle) return;
	dbgk_align_timing now;
	dbgk_align_timing_get(handle, &now);
	if (getenv("DBGK_TIMINGS"))
		cerr << "Contig stage aligned arms (bubbles): candidates " << n_candidates << " submitted " << submitted.size() / 2 << " too long " << n_too_long
		     << " used " << n_align_used << " aligned on the host " << n_align_host << " device ms " << now.ms_align - before.ms_align
		     << " bytes copied back " << now.bytes_back - before.bytes_back << endl;
	before = now;
}

// After a pass: the device copy gets what the pass changed; the pass's line under DBGK_TIMINGS
static int end_pass(const char *name, dbgk_simplify_timing &before)
{
	if (!handle) return 0;
	const int rc = dbgk_simplify_update(handle, dirty.data(), dirty.size());
	if (rc) return gpu_failed(rc);
	dbgk_simplify_timing now;
	dbgk_simplify_timing_get(handle, &now);
	if (getenv("DBGK_TIMINGS"))
		cerr << "Contig stage traced paths (" << name << "): requests " << (have_traces ? rows.size() : 0) << " traces used " << n_used
		     << " fell back to the host walk " << n_fell_back << " device ms "
		     << (now.ms_trace + now.ms_branches + now.ms_fill + now.ms_update) - (before.ms_trace + before.ms_branches + before.ms_fill + before.ms_update)
		     << " bytes copied back " << now.bytes_returned - before.bytes_returned << endl;
	before = now;
	have_traces = false;
	return 0;
}
// array[G::size()].kmer, which the reference prints for an end without a node (:344, :1006): the word behind its table, 0 there
static std::string kmer_at(uint64_t i) { return G::decimal(i == G::size() ? (Key)0 : G::kmer(i)); }

// canonical form of a neighbour k-mer; flipped says that it is the reverse complement
static Key canonical(Key kmer, bool &flipped)
{
	const Key rc = G::rev_com(kmer);
	flipped = !(kmer < rc);
	return flipped ? rc : kmer;
}

// calculate_kmer_links (:107-181) on the host, for a table that did not get its link records from the device
static void first_pass_host(std::vector<uint64_t> &tips, std::vector<uint64_t> &branches)
{
	for (uint64_t i = 0; i < G::size(); i++) {
		if (is_entity_null(G::nul_flag(), i)) continue;
		int num[2] = {0, 0}, base[2] = {0, 0};
		for (int side = 0; side < 2; side++) {
			const uint32_t link = side ? G::r_link(i) : G::l_link(i);
			int max_depth = 0;
			for (int j = 0; j < 4; j++) {
				const int depth = get_next_kmer_depth(link, j);
				if (depth > KmerFreqCutoff) {
					if (num[side] < 3) num[side]++;
					if (max_depth < depth) {
						max_depth = depth;
						base[side] = j;
					}
				}
			}
		}
		klink[i] = (uint16_t)(num[0] | base[0] << 2 | num[1] << 4 | base[1] << 6 | ((num[0] == 1 && num[1] == 1) ? 0x100 : 0));
		if (num[0] == 0 && num[1] == 0) set_entity_delete(G::del_flag(), i);
		if (num[0] + num[1] == 1) tips.push_back(i);
		if (num[0] > 1 || num[1] > 1) branches.push_back(i);
	}
}

// recalculate_kmer_links, :210-277: a link whose neighbour is gone is cleared in the node itself
static void recalculate(uint64_t idx)
{
	if (idx == G::size()) return;
	mark_changed(idx);
	const Key kmer = G::kmer(idx);
	int num[2] = {0, 0}, base[2] = {0, 0};
	for (int side = 0; side < 2; side++) {
		uint32_t &link = side ? G::r_link(idx) : G::l_link(idx);
		int max_depth = 0;
		for (int j = 0; j < 4; j++) {
			const int depth = get_next_kmer_depth(link, j);
			if (depth <= KmerFreqCutoff) continue;
			bool flipped;
			const Key key = canonical(side ? G::next_rightward(kmer, j) : G::next_leftward(kmer, j), flipped);
			if (G::exist(key) != G::size()) {
				if (num[side] < 3) num[side]++;
				if (max_depth < depth) {
					max_depth = depth;
					base[side] = j;
				}
			} else {
				link &= kClearBase[j];
			}
		}
	}
	klink[idx] = (uint16_t)((klink[idx] & 0xFE00) | num[0] | base[0] << 2 | num[1] << 4 | base[1] << 6 | ((num[0] == 1 && num[1] == 1) ? 0x100 : 0));
}

// get_linear_path, :779-827: from idx along the strongest link until a node that is not linear, no node, or len_cutoff steps
static void linear_path(uint64_t idx, int direct, int len_cutoff, Path &p)
{
	const int original = direct;
	for (;;) {
		p.len++;
		p.nodes.push_back(idx);
		const Key kmer = G::kmer(idx);
		Key next;
		if (direct == 1) {
			next = G::next_rightward(kmer, r_base(idx));
			p.depth += get_next_kmer_depth(G::r_link(idx), r_base(idx));
			p.str.push_back(original == 1 ? bases[r_base(idx)] : c_bases[r_base(idx)]);
		} else {
			next = G::next_leftward(kmer, l_base(idx));
			p.depth += get_next_kmer_depth(G::l_link(idx), l_base(idx));
			p.str.push_back(original == 1 ? c_bases[l_base(idx)] : bases[l_base(idx)]);
		}
		bool flipped;
		const Key key = canonical(next, flipped);
		if (flipped) direct = -direct;
		idx = G::exist(key);
		if (!is_linear(idx) || p.len >= len_cutoff) {
			p.last = idx;
			if (idx == G::size()) p.mark = "break";
			else p.mark = (l_num(idx) == 0 || r_num(idx) == 0) ? "break" : "branch";
			return;
		}
	}
}

// linear_path(idx, direct, len_cutoff, p), from the pass's trace where that still holds.  row: the request's (a tip), or
// 8 i + 4 side + j for base j on the right (side 0) or left of branching node i; branch: that node, or size() for a tip.  The trace
// is the walk if and only if the branching node is unchanged (its row was derived from its link words), the row starts where the
// host just found the walk to start, in that direction, and no node of the path and not its last slot has changed; every slot a
// walk reads beyond those -- the probe chains it passes -- holds keys and filled bits, which no pass changes.
static void traced_or_walked(uint64_t row, uint64_t branch, uint64_t idx, int direct, int len_cutoff, Path &p)
{
	if (have_traces) {
		const dbgk_trace_row &r = rows[row];
		bool ok = r.status == DBGK_TRACE_TRACED && r.len > 0 && r.start == idx && r.direct == direct && (branch == G::size() || !is_changed(branch)) &&
		          (r.last == G::size() || !is_changed(r.last));
		for (uint64_t j = node_first[row]; ok && j < node_first[row + 1]; j++) ok = !is_changed(trace_nodes[j]);
		if (ok) {
			n_used++;
			p.len = (int)r.len;
			p.depth = (int)r.depth;
			p.last = r.last;
			p.mark = r.mark ? "branch" : "break";
			p.nodes.assign(trace_nodes.begin() + node_first[row], trace_nodes.begin() + node_first[row + 1]);
			p.str.resize(r.len);
			for (uint32_t j = 0; j < r.len; j++) p.str[j] = bases[trace_bases[node_first[row] + j]];
			return;
		}
		n_fell_back++;
	}
	linear_path(idx, direct, len_cutoff, p);
}

static void delete_nodes(const std::vector<uint64_t> &nodes)
{
	for (uint64_t v : nodes) {
		set_entity_delete(G::del_flag(), v);
		mark_changed(v);
	}
}

// the path as it reads from left to right: k-mer of its first node in front of, or behind, the steps' bases (:335-342)
static std::string path_sequence(uint64_t first_node, int direct, std::string steps)
{
	const std::string kmer = G::text(G::kmer(first_node));
	if (direct == 1) return kmer + steps;
	std::reverse(steps.begin(), steps.end());
	return steps + kmer;
}

// remove_error_tips, :281-355
static void remove_tips(const std::vector<uint64_t> &tips)
{
	uint64_t total_num = 0, total_len = 0;
	const string path = Output_prefix + ".contig.tip.fa";
	ofstream out(path.c_str());
	if (!out) cerr << "fail to open file " << path << endl;
	for (size_t i = 0; i < tips.size(); i++) {
		const uint64_t idx = tips[i];
		const int direct = (l_num(idx) == 1) ? -1 : 1;
		Path p;
		traced_or_walked(i, G::size(), idx, direct, Tip_len_cutoff, p);
		const double avg = (double)p.depth / p.len;
		if (!(avg <= Tip_depth_cutoff && p.len <= Tip_len_cutoff)) continue;
		total_num++;
		total_len += p.len;
		delete_nodes(p.nodes);
		recalculate(p.last);
		set_flag(p.last, IN_TIP);
		const std::string left_kmer = direct == 1 ? G::decimal(G::kmer(idx)) : kmer_at(p.last), right_kmer = direct == 1 ? kmer_at(p.last) : G::decimal(G::kmer(idx));
		const char *left_mark = direct == 1 ? "break" : p.mark, *right_mark = direct == 1 ? p.mark : "break";
		out << ">tip_" << total_num << "\tlength: " << p.len + KmerSize << "\tavgDepth: " << avg << "\tLeftEndKmer: " << left_kmer << " " << left_mark
		    << "\tRightEndKmer: " << right_kmer << " " << right_mark << "\n" << path_sequence(idx, direct, p.str) << "\n";
	}
	out.close();
	cerr << "\nremove total tip number:  " << total_num << endl;
	cerr << "remove total tip length:  " << total_len << endl;
}

// remove_lowCov_edges, :601-776: rightward edges of a branching node first, then its leftward ones (whose header line is spelt
// differently, :763)
static void remove_low_edges(const std::vector<uint64_t> &branches)
{
	int total_num = 0, total_len = 0;
	const string path = Output_prefix + ".contig.lowedge.fa";
	ofstream out(path.c_str());
	if (!out) cerr << "fail to open file " << path << endl;
	for (size_t i = 0; i < branches.size(); i++) {
		const uint64_t idx = branches[i];
		for (int direct = 1; direct >= -1; direct -= 2) {
			if ((direct == 1 ? r_num(idx) : l_num(idx)) < 2) continue;
			std::vector<uint8_t> vb, vd;
			branch_bases(direct == 1 ? G::r_link(idx) : G::l_link(idx), vb, vd);
			for (size_t j = 0; j < vb.size(); j++) {
				bool flipped;
				const Key key = canonical(direct == 1 ? G::next_rightward(G::kmer(idx), vb[j]) : G::next_leftward(G::kmer(idx), vb[j]), flipped);
				const int direct1 = flipped ? -direct : direct;
				const uint64_t idx1 = G::exist(key);
				if (!is_linear(idx1)) continue;
				Path p;
				traced_or_walked(8 * i + (direct == 1 ? 0 : 4) + vb[j], idx, idx1, direct1, LowCovEdge_len_cutoff, p);
				const int len = p.len + 1, depth = p.depth + vd[j];
				const double avg = (double)depth / len;
				if (!(len <= LowCovEdge_len_cutoff && avg <= LowCovEdge_depth_cutoff && !is_linear(p.last))) continue;
				total_num++;
				total_len += len;
				delete_nodes(p.nodes);
				recalculate(p.last);
				recalculate(idx);
				set_flag(idx, IN_LOWEDGE);
				set_flag(p.last, IN_LOWEDGE);
				const std::string seq = path_sequence(idx1, direct1, p.str);
				if (direct == 1)
					out << ">lowedge_" << total_num << "\tlength: " << len + KmerSize << "\tavgDepth: " << avg << "\tLeftEndKmer: " << G::decimal(G::kmer(idx))
					    << " branch" << "\tRightEndKmer: " << kmer_at(p.last) << " " << p.mark << "\n" << seq << "\n";
				else
					out << ">lowedge_" << total_num << "    length:" << len + KmerSize << "    avgDepth:" << avg << "\tLeftEndKmer: " << kmer_at(p.last) << " "
					    << p.mark << "\tRightEndKmer: " << G::decimal(G::kmer(idx)) << " branch" << "\n" << seq << "\n";
			}
		}
	}
	cerr << "\nremove total lowCovEdge number: " << total_num << endl;
	cerr << "remove total lowCovEdge length: " << total_len << endl;
	out.close();
}

// remove_hetero_bubbles, :375-582
static void remove_bubbles(const std::vector<uint64_t> &branches)
{
	const string path = Output_prefix + ".contig.bubble.fa";
	ofstream out(path.c_str());
	if (!out) cerr << "fail to open file " << path << endl;
	uint64_t total_num = 0, total_len = 0;
	for (size_t i = 0; i < branches.size(); i++) {
		const uint64_t idx = branches[i];
		int direct = 0;
		std::vector<uint8_t> vb, vd;
		if (l_num(idx) == 2 && r_num(idx) == 1) {
			direct = -1;
			branch_bases(G::l_link(idx), vb, vd);
		} else if (l_num(idx) == 1 && r_num(idx) == 2) {
			direct = 1;
			branch_bases(G::r_link(idx), vb, vd);
		} else {
			continue;
		}
		uint64_t first[2];
		int dir[2];
		for (int e = 0; e < 2; e++) {
			bool flipped;
			const Key key = canonical(direct == 1 ? G::next_rightward(G::kmer(idx), vb[e]) : G::next_leftward(G::kmer(idx), vb[e]), flipped);
			dir[e] = flipped ? -direct : direct;
			first[e] = G::exist(key);
		}
		if (!is_linear(first[0]) || !is_linear(first[1])) continue;
		Path p[2];
		for (int e = 0; e < 2; e++) traced_or_walked(8 * i + (direct == 1 ? 0 : 4) + vb[e], idx, first[e], dir[e], Bubble_len_cutoff, p[e]);
		const double avg1 = (double)p[0].depth / p[0].len, avg2 = (double)p[1].depth / p[1].len;
		if (p[0].last != p[1].last) {
			if (avg1 > LowCovEdge_depth_cutoff && avg2 > LowCovEdge_depth_cutoff) set_flag(idx, IN_REPEAT);   // a tiny repeat, no bubble (:471-473)
			continue;
		}
		std::string s1 = path_sequence(first[0], dir[0], p[0].str), s2 = path_sequence(first[1], dir[1], p[1].str);
		if (dir[0] != dir[1]) {      // :494-497
			std::reverse(s1.begin(), s1.end());
			complement_sequence(s1);
		}
		const int len1 = p[0].len + 1, len2 = p[1].len + 1;   // the branching base counts (:500-503)
		double diff_rate = 0;
		const char *type = "";
		if (len1 == len2) {
			diff_rate = (double)count_differences(s1, s2) / len1;
			type = "SNP";
		}
		if (len1 != len2 || diff_rate > Bubble_base_diff_rate_cutoff) {
			std::string a1, a2;
			aligned_arms(i, s1, s2, a1, a2);
			s1 = a1;
			s2 = a2;
			diff_rate = (double)count_differences(s1, s2) / len1;
			type = "INDEL";
		}
		if (!(diff_rate < Bubble_base_diff_rate_cutoff && abs(len1 - len2) < Bubble_len_cutoff * Bubble_len_diff_rate_cutoff &&
		      (len1 <= Bubble_len_cutoff && len2 <= Bubble_len_cutoff)))
			continue;
		const int removed = avg1 < avg2 ? 1 : 2;            // the branch of lower depth goes (:531-551)
		delete_nodes(p[removed - 1].nodes);
		recalculate(p[removed - 1].last);
		recalculate(idx);
		total_num++;
		total_len += removed == 1 ? len1 : len2;
		const std::string left_kmer = direct == 1 ? G::decimal(G::kmer(idx)) : kmer_at(p[0].last), right_kmer = direct == 1 ? kmer_at(p[0].last) : G::decimal(G::kmer(idx));
		const char *left_mark = direct == 1 ? "branch" : p[0].mark, *right_mark = direct == 1 ? p[0].mark : "branch";
		out << ">bubble_" << total_num << "\ttype: " << type << "\tlength1: " << len1 + KmerSize << "\tavgDepth1: " << avg1 << "\tlength2: " << len2 + KmerSize
		    << "\tavgDepth2: " << avg2 << "\tremoved: " << removed << "\tLeftEndKmer: " << left_kmer << " " << left_mark << "\tRightEndKmer: " << right_kmer
		    << " " << right_mark << "\n" << s1 << "\n" << s2 << "\n";
		set_flag(idx, IN_BUBBLE);
		set_flag(p[0].last, IN_BUBBLE);
	}
	cerr << "\nremove total bubble number: " << total_num << endl;
	cerr << "remove total bubble length: " << total_len << endl;
	out.close();
}

// read_out_contig, :900-1046: the contigs come from the GPU in the order of the reference's scan
static int read_out(double &ms_gpu, double &ms_files)
{
	const string seq_path = Output_prefix + ".contig.seq.fa", depth_path = Output_prefix + ".contig.seq.depth";
	ofstream seq_out(seq_path.c_str()), depth_out(depth_path.c_str());
	if (!seq_out || !depth_out) cerr << "fail to open contig file " << seq_path << "\t" << depth_path << endl;
	const string small_path = Output_prefix + ".contig.small.fa", small_depth_path = Output_prefix + ".contig.small.depth";
	ofstream small_out(small_path.c_str()), small_depth_out(small_depth_path.c_str());
	if (!small_out || !small_depth_out) cerr << "fail to open small file " << small_path << "\t" << small_depth_path << endl;

	auto t0 = std::chrono::steady_clock::now();
	// the passes' handle, whose device copy they kept equal to the host arrays; without one (no pass, or simplify_host) the table goes up here
	dbgk_contig_summary sum;
	int rc = handle ? 0 : open_handle();
	dbgk_contig *h = handle;
	handle = NULL;
	if (!rc) rc = dbgk_contig_read_out(h, &sum);
	if (rc) {
		cerr << "contig read-out on the GPU failed: " << dbgk_strerror(rc) << " " << dbgk_last_error() << endl;
		if (h) dbgk_contig_destroy(h);
		return rc;
	}
	std::vector<uint64_t> off(sum.contigs + 1);
	std::vector<dbgk_contig_record> rec(sum.contigs);
	std::string seqs(sum.bytes, '\0'), depths(sum.bytes, '\0');
	dbgk_contig_results(h, off.data(), rec.data(), &seqs[0], &depths[0]);
	dbgk_contig_timing tm;
	dbgk_contig_timing_get(h, &tm);
	dbgk_contig_destroy(h);
	ms_gpu = ms_since(t0);
	if (getenv("DBGK_TIMINGS"))
		cerr << "Contig read-out (ms): upload " << tm.ms_upload << " (" << tm.upload_bytes << " bytes) compact " << tm.ms_compact << " successors "
		     << tm.ms_successors << " mutual " << tm.ms_mutual << " rank " << tm.ms_rank << " (" << sum.rounds << " rounds) place " << tm.ms_place
		     << " scatter " << tm.ms_scatter << " emit " << tm.ms_emit << " host walk " << tm.ms_host_walk << "; contigs by kernels "
		     << sum.kernel_contigs << ", by the host walker " << sum.host_contigs << endl;

	t0 = std::chrono::steady_clock::now();
	static const char *const kMark[2] = {"break", "branch"}, *const kRepeat[3] = {"Unknown", "Unique", "Repeat"};
	uint64_t break_points = 0, branch_points = 0;
	std::vector<std::string> header(sum.contigs);
	std::vector<std::pair<uint64_t, uint64_t>> order(sum.contigs);   // (length, index in scan order)
	for (uint64_t i = 0; i < sum.contigs; i++) {
		const dbgk_contig_record &r = rec[i];
		const int contig_len = (int)r.left_len + KmerSize + (int)r.right_len;
		double avg = (int)r.left_depth + (int)r.right_depth;
		avg /= (double)((int)r.left_len + (int)r.right_len);
		(r.right_mark ? branch_points : break_points)++;
		(r.left_mark ? branch_points : break_points)++;
		char num[64];
		snprintf(num, sizeof num, "%.17g", avg);       // boost::lexical_cast<string>(double), :1006
		header[i] = "\tlength: " + std::to_string(contig_len) + "\tavgDepth: " + num + "\tLeftEndKmer: " + kmer_at(r.left_end) + " " +
		            kMark[r.left_mark] + "-" + kRepeat[r.left_repeat] + "\tRightEndKmer: " + kmer_at(r.right_end) + " " + kMark[r.right_mark] +
		            "-" + kRepeat[r.right_repeat] + "\t" + ((r.left_repeat == 2 && r.right_repeat == 2) ? "RepeatNode" : "") + "\n";
		order[i] = std::make_pair(off[i + 1] - off[i], i);
	}
	// the reference sorts its records with std::sort and cmpSeqByLen (:48-50, :1014): the same algorithm with the same
	// comparisons leaves equal lengths in the same places
	std::sort(order.begin(), order.end(), [](std::pair<uint64_t, uint64_t> a, std::pair<uint64_t, uint64_t> b) { return b.first < a.first; });
	uint64_t contig_num = 0, contig_len = 0, small_num = 0, small_len = 0, id = 1;
	for (const auto &o : order) {
		const uint64_t i = o.second, len = o.first;
		const bool big = len >= (uint64_t)Contig_len_cutoff;
		ofstream &fa = big ? seq_out : small_out, &dp = big ? depth_out : small_depth_out;
		fa << ">ctg_" << id << header[i];
		fa.write(&seqs[off[i]], len);
		fa << "\n";
		dp << ">ctg_" << id << "\n";
		dp.write(&depths[off[i]], len);
		dp << "\n";
		(big ? contig_num : small_num)++;
		(big ? contig_len : small_len) += len;
		id += 2;
	}
	cerr << "\ncontig break-point number:     " << break_points << endl;
	cerr << "contig branch-point number:    " << branch_points << endl;
	cerr << "\nTotal contig number:   " << contig_num << endl;
	cerr << "Total contig length:   " << contig_len << endl;
	cerr << "\nTotal small edge number:   " << small_num << endl;
	cerr << "Total small edge length:   " << small_len << endl;
	ms_files = ms_since(t0);
	return 0;
}

// build_contig_sequence, :54-102
static int run()
{
	double ms_first = 0, ms_tip = 0, ms_edge = 0, ms_bubble = 0, ms_gpu = 0, ms_files = 0;
	dbgk_simplify_timing traced_so_far = {};
	dbgk_align_timing aligned_so_far = {};
	cerr << "\nStart to calulate kmer links information!" << endl;
	if (sizeof(Key) > 8) cerr << "Contig stage on 128-bit k-mers (32-byte nodes; parity unpinned above k = 32)" << endl;
	auto t0 = std::chrono::steady_clock::now();
	std::vector<uint64_t> tips, branches;
	if (DbgkKmerLinks) {             // the first pass came with the table, computed on the device (dbgk_export_host_table_links, dbgk_wide_export_host_table_links)
		klink = DbgkKmerLinks;
		tips.swap(DbgkTipNodes);
		branches.swap(DbgkBranchNodes);
	} else {                         // a table laid out on the host (DBGK_LAYOUT=ref: its slots are not the device table's) or DBGK_LINKS=0: the same pass here.
		                                 // The records live until the program leaves (main.cpp leaves through _exit): never freed
		klink = static_cast<uint16_t *>(calloc(G::size(), sizeof(uint16_t)));
		if (!klink) return DBGK_ERR_NOMEM;
		first_pass_host(tips, branches);
	}
	write_kmer_freq_file(Output_prefix + ".contig.kmer.freq", KmerFreqCutoff);   // the five counts and the file, :186-203
	ms_first = ms_since(t0);
	finished("Finished!");

	if (is_remove_tip) {
		cerr << "\nStart to remove tips caused by sequencing error!" << endl;
		t0 = std::chrono::steady_clock::now();
		if (int rc = begin_pass(tips, true, Tip_len_cutoff)) return rc;
		remove_tips(tips);
		if (int rc = end_pass("tips", traced_so_far)) return rc;
		ms_tip = ms_since(t0);
		finished("Finished!");
	}
	if (is_remove_lowedge) {
		cerr << "\nStart to remove small low coverage edges between two branching nodes!" << endl;
		t0 = std::chrono::steady_clock::now();
		if (int rc = begin_pass(branches, false, LowCovEdge_len_cutoff)) return rc;
		remove_low_edges(branches);
		if (int rc = end_pass("low edges", traced_so_far)) return rc;
		ms_edge = ms_since(t0);
		finished("Finshed!");        // :82
	}
	if (is_remove_bubble) {
		cerr << "\nStart to remove bubbles caused by repeats and heterozygotes!" << endl;
		t0 = std::chrono::steady_clock::now();
		if (int rc = begin_pass(branches, false, Bubble_len_cutoff)) return rc;
		if (int rc = collect_alignments(branches)) return rc;
		remove_bubbles(branches);
		if (int rc = end_pass("bubbles", traced_so_far)) return rc;
		report_alignments(aligned_so_far);
		ms_bubble = ms_since(t0);
		finished("Finished!");
	}
	cerr << "\nStart to read out contig sequence and the depth information!" << endl;
	const int rc = read_out(ms_gpu, ms_files);
	if (rc) return rc;
	finished("Finished!");
	if (getenv("DBGK_TIMINGS"))
		cerr << "Contig stage host passes (ms): first pass " << ms_first << " tips " << ms_tip << " low edges " << ms_edge << " bubbles " << ms_bubble
		     << " read-out " << ms_gpu << " headers, sort and files " << ms_files << endl;
	return 0;
}
};   // Stage

template <class G> dbgk_contig *Stage<G>::handle = NULL;
template <class G> bool Stage<G>::have_traces = false;
template <class G> std::vector<dbgk_trace_row> Stage<G>::rows;
template <class G> std::vector<uint64_t> Stage<G>::node_first;
template <class G> std::vector<uint32_t> Stage<G>::trace_nodes;
template <class G> std::vector<uint8_t> Stage<G>::trace_bases;
template <class G> std::vector<uint8_t> Stage<G>::changed;
template <class G> std::vector<uint64_t> Stage<G>::dirty;
template <class G> uint64_t Stage<G>::n_used = 0;
template <class G> uint64_t Stage<G>::n_fell_back = 0;
template <class G> std::vector<int64_t> Stage<G>::pair_of;
template <class G> std::vector<std::string> Stage<G>::submitted;
template <class G> std::vector<dbgk_align_row> Stage<G>::align_rows;
template <class G> std::vector<uint64_t> Stage<G>::align_first;
template <class G> std::string Stage<G>::align_i;
template <class G> std::string Stage<G>::align_j;
template <class G> uint64_t Stage<G>::n_candidates = 0;
template <class G> uint64_t Stage<G>::n_too_long = 0;
template <class G> uint64_t Stage<G>::n_align_used = 0;
template <class G> uint64_t Stage<G>::n_align_host = 0;

} // namespace

int run_contig_stage() { return Stage<Keys64>::run(); }

int run_contig_stage_wide() { return Stage<Keys128>::run(); }

// test hook contig_wide: `kset` carried over to 32-byte nodes with a high word of 0 -- the same slots, flags and link words
// (hash_code128(0, lo) == hash_code(lo), so every key sits where a 128-bit probe looks for it) -- and the wide stage on that
int run_contig_stage_wide_on_kset()
{
	const uint64_t size = kset->size, flag_bytes = size / 8 + 1;
	KmerNode32 *array = static_cast<KmerNode32 *>(kmerset_alloc(size * sizeof(KmerNode32), true));
	uint8_t *nul = static_cast<uint8_t *>(kmerset_alloc(flag_bytes, false)), *del = static_cast<uint8_t *>(kmerset_alloc(flag_bytes, false));
	if (!array || !nul || !del) {
		free(array), free(nul), free(del);
		return DBGK_ERR_NOMEM;
	}
	for (uint64_t i = 0; i < size; i++) {
		array[i].kmer_lo = kset->array[i].kmer;
		array[i].l_link = kset->array[i].l_link;
		array[i].r_link = kset->array[i].r_link;
	}
	memcpy(nul, kset->nul_flag, flag_bytes);
	memcpy(del, kset->del_flag, flag_bytes);
	if (kset_wide) free_hash128(kset_wide);
	kset_wide = adopt_kmerset128(size, kset->load_factor, kset->count, kset->count_conflict, array, nul, del);
	if (!kset_wide) return DBGK_ERR_NOMEM;
	return run_contig_stage_wide();
}
