/*
 * dbgk.h -- C ABI of the MI355X (gfx950) k-mer / de Bruijn graph construction layer.
 *
 * This is the drop-in boundary underneath DBG_assembly's build_debruijn_graph()
 * (reference: DBG_contig/DBGgraph.h:66, DBG_contig/DBGgraph.cpp:364-430).  The reference has no
 * FFI of its own (single C++ process); the entry points below are what
 * its hot path decomposes into when the compute moves to the GPU.  Each one names the reference
 * routine it replaces.  All functions are extern "C", take plain pointers and sizes, return an
 * int status (0 = DBGK_OK, < 0 = error, never hang on a full table) and may be called from one
 * host thread per handle.  One handle = one GPU = one HIP stream.
 *
 * There is NO CPU fallback behind this interface: every entry point fails with DBGK_ERR_HIP when
 * no gfx950 device is usable.
 *
 * Paths are relative to /root/reference/.
 */
#ifndef DBGK_H_
#define DBGK_H_

#include <stddef.h>
#include <stdint.h>
#include "dbgk_synth.h"
#include "dbgk_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBGK_ABI_VERSION 7

/* status codes */
#define DBGK_OK               0
#define DBGK_ERR_ARG         -1   /* bad argument / unsupported parameter (k < 1 or k > 32, ...)    */
#define DBGK_ERR_HIP         -2   /* HIP runtime error or no gfx950 device; see dbgk_last_error()    */
#define DBGK_ERR_TABLE_FULL  -3   /* an insert found no free slot: the reference would spin forever
                                     here (DBGgraph.cpp:170-205); create a larger handle            */
#define DBGK_ERR_STATE       -4   /* call order violated (push after finalize, export before, ...)  */
#define DBGK_ERR_NOMEM       -5   /* device or host allocation failed                               */
#define DBGK_ERR_CAPACITY    -6   /* caller-provided output buffer too small                        */

/* the 16-byte graph node: bit-identical to KmerNode (DBG_contig/kmerSet.h:70-75).  Each link word
 * holds four saturating 8-bit counters, A in bits 31..24 ... T in bits 7..0 (kmerSet.cpp:56).      */
typedef struct dbgk_node {
	uint64_t kmer;
	uint32_t l_link;
	uint32_t r_link;
} dbgk_node;

typedef struct dbgk_handle dbgk_handle;

/* engine selection for the insert path */
#define DBGK_ENGINE_AUTO       0
#define DBGK_ENGINE_DIRECT     1  /* fused extract + 64-bit-atomic insert into the global table      */
#define DBGK_ENGINE_PARTITION  2  /* extract -> radix-partitioned records -> LDS-built table regions */
#define DBGK_ENGINE_SEEDIDX    4  /* link_scaffold's seed index: every k-mer of the pushed CONTIGS -> (contig
                                     index, position, strand) of its first occurrence + uniqueness flag   */
#define DBGK_ENGINE_WIDE       5  /* k-mers of up to 63 bases: 128-bit keys, 32-byte nodes (include/dbgk_wide.h; the reference
                                     stops at k = 31, so this path is this build's own definition: parity unpinned for
                                     k > 32, identical to the reference's rules for k <= 32).  expected_kmers > 0 and
                                     2^26 <= table_slots < 2^34: 16-byte records are radix-partitioned and the table is built
                                     region by region in LDS (2.7x faster; 16 bytes per occurrence of a pass + an eighth again
                                     must fit the device; with one shard and one pass what does not fit the record store joins
                                     through the atomic kernels after the build); otherwise fused extract + atomic insert.
                                     shard_count >= 1: slot-range shards of ONE table like the 64-bit engine (dbgk_shard_*);
                                     big tables / small devices: several passes over the input (dbgk_wide_begin_pass).
                                     Results through dbgk_wide_export_*, dbgk_digest, dbgk_link_stats_device            */
#define DBGK_ENGINE_KFREQ      3  /* no graph: direct-addressed 4^k table of saturating 8-bit counts of
                                     canonical k-mers (the correct_error module's frequency table);
                                     table_slots is ignored, k <= 18.  expected_kmers > 0: the occurrences
                                     are partitioned and aggregated in LDS (2.6x faster; 8 bytes per
                                     occurrence must fit the device), 0: atomics on the table, any size */

typedef struct dbgk_config {
	int32_t  kmer_size;        /* KmerSize   (DBGgraph.cpp:10), 1..32 (1..63 with DBGK_ENGINE_WIDE)     */
	int32_t  max_read_len;     /* maxReadLen (DBGgraph.cpp:11): longer reads are trimmed           */
	uint64_t table_slots;      /* number of 16-byte slots of the device table == kset->size the
	                              host wants (a "prime" from find_next_prime, kmerSet.cpp:85-95);
	                              slot of a key = hash_code(key) % table_slots (DBGgraph.cpp:167) */
	int32_t  device_id;        /* HIP device ordinal                                               */
	int32_t  engine;           /* DBGK_ENGINE_*                                                    */
	uint64_t max_batch_bases;  /* capacity of the internal staging buffers used by
	                              dbgk_push_reads (host buffers); 0 = default (256 MiB)            */
	uint64_t expected_kmers;   /* PARTITION engine: k-mer occurrences the record store is sized for
	                              (8 bytes each, twice).  Input of unknown size streams through it:
	                              a push that would not fit is preceded by a flush (dbgk_flush), which
	                              merges the stored records into the table.  A job that fits is built
	                              in one go at finalize (fastest).  0 = derive from table_slots      */
	uint32_t shard_count;      /* > 1: this handle is one of shard_count handles (one per GPU) that
	                              together hold ONE table of table_slots slots, each a contiguous
	                              slot range; 0 = unsharded (1 = a single shard that still follows
	                              the exchange protocol, useful for testing it on one GPU)        */
	uint32_t shard_index;      /* 0 .. shard_count-1                                               */
	uint64_t flags;            /* DBGK_FLAG_*                                                      */
	uint64_t n_passes;         /* DBGK_ENGINE_WIDE through records: read the input (at least) this many times, every
	                              pass keeping the records of a part of the level-1 buckets (dbgk_wide_begin_pass);
	                              the geometry may need more (a pass fans out to at most 1024 level-1 buckets, counted
	                              over all shards): ask dbgk_wide_pass_info.  0 on an unsharded handle = the plain
	                              create / push / finalize flow, never the pass protocol: a table one pass cannot
	                              cover is then built by the atomic kernels.  0 on a sharded handle = as few as needed */
	uint64_t reserved[1];
} dbgk_config;

/* DIRECT engine only: remember for every key the position (in pushed bases, over all pushes) of its
 * first occurrence, so that dbgk_export_first_seen_order can list the nodes in the order in which
 * the reference's single-threaded path first inserts them (DBGgraph.cpp:139-205 at -t 1).  Costs one
 * extra 64-bit atomic per k-mer and 8 bytes per slot.                                            */
#define DBGK_FLAG_TRACK_FIRST_SEEN 1ull
/* allocate the two pinned staging buffers (max_batch_bases each + offsets) and their device twins inside dbgk_create instead of on the
 * first dbgk_push_reads / dbgk_push_acquire: page-locking a few hundred MB costs tens of milliseconds, which a host that creates the
 * handle on a thread beside its first file read hides this way (host/DBGgraph.cpp)                                               */
#define DBGK_FLAG_PREALLOC_STAGING 2ull

/* totals after dbgk_finalize (the globals the reference prints, DBGgraph.cpp:410-411, and the
 * KmerSet counters of kmerSet.cpp:331-338) */
typedef struct dbgk_stats {
	uint64_t total_reads;      /* Total_reads_num: every record pushed, also too-short ones (:274) */
	uint64_t total_kmers;      /* Kmer_total_num : sum of (len-K+1) over reads with len >= K,
	                              UNtrimmed length (:101)                                          */
	uint64_t stored_kmers;     /* windows actually extracted = sum max(0,min(len,maxReadLen)-K+1);
	                              the unit of BASELINE.json's metric                               */
	uint64_t count;            /* kset->count: distinct keys INCLUDING the key-0 node (:418)       */
	uint64_t count_conflict;   /* probe steps taken (layout dependent, informational)              */
	uint64_t table_slots;
	uint32_t polyA_l_link;     /* links of the key-0 (poly-A / poly-T) node (:153-164)             */
	uint32_t polyA_r_link;
	uint64_t other_bytes;      /* sequence bytes that are none of ACGTNacgtn.  The reference maps them to
	                              4 and then reads out of bounds (seqKmer.cpp:9-19, DBGgraph.cpp:71-73);
	                              here EVERY engine reads them as 'A', like N, and counts them (ABI 5) */
} dbgk_stats;

/* first pass of the consumer (DBG_contig/contig.cpp:107-181) computed on the device table */
typedef struct dbgk_link_stats {
	int64_t depth_stat[256];   /* DepthStat: histogram of all 8 counters of every node            */
	int64_t total_nodes;
	int64_t deleted_lowfreq;   /* nodes with no counter > cutoff on either side                    */
	int64_t linear_nodes;      /* exactly one on each side                                         */
	int64_t tip_nodes;         /* l+r == 1                                                         */
	int64_t branch_nodes;      /* l > 1 or r > 1                                                   */
} dbgk_link_stats;

/* per-phase device timings of the most recent push/finalize, from HIP events on the handle's
 * stream (milliseconds; 0 when the phase did not run) */
typedef struct dbgk_timings {
	float mark_ms;             /* read-boundary bitmap + totals                                    */
	float insert_ms;           /* DIRECT: fused extract+insert kernel; PARTITION: extract+scatter  */
	float partition_ms;        /* PARTITION: second-level scatter                                  */
	float build_ms;            /* PARTITION: LDS region build + emit                               */
	float fixup_ms;            /* PARTITION: overflow records through the direct path              */
	float finalize_ms;         /* key-0 node, flags, count reduce                                  */
	uint64_t insert_launches;  /* number of launches accumulated into insert_ms                    */
	float l2_build_wall_ms;    /* PARTITION: wall time of the second-level scatter and the region build
	                              together; they run concurrently on two streams, so partition_ms and
	                              build_ms (sums of their launches) overlap and add up to more than this */
	uint32_t partition_launches; /* launches accumulated into partition_ms (= into build_ms)         */
	uint32_t uniform_launches;   /* of insert_launches: batches of equal-length reads, which take the
	                                PARTITION engine's k_extract_scatter_uniform instead of k_extract_scatter */
	uint32_t prefix_launches;    /* of insert_launches: batches of mixed-length reads through k_extract_scatter_prefix (every read
	                                exactly the lanes its windows need; dbgk_partition.h)                                          */
	uint64_t reserved[1];
} dbgk_timings;

/* ---- life cycle ------------------------------------------------------------------------------ */

/* replaces init_kmerset_parallel + the staging allocations of build_debruijn_graph
 * (kmerSet.cpp:98-127, DBGgraph.cpp:381-402): allocates and zeroes the device table.            */
int dbgk_create(const dbgk_config *cfg, dbgk_handle **out);
int dbgk_destroy(dbgk_handle *h);
/* back to the state right after dbgk_create (table zeroed, totals cleared) without reallocating */
int dbgk_reset(dbgk_handle *h);

/* ---- the hot path ------------------------------------------------------------------------------ */

/* replaces one block iteration of parse_one_reads_file: thread_parseBlock + thread_updatekmers
 * (DBGgraph.cpp:38-120,126-213) for `n_reads` reads.  bases = the sequences back to back with no
 * separators (ASCII; ACGT in either case, N / n counts as A like seqKmer.cpp:9-19; any other byte -- IUPAC codes,
 * '-', '*', bytes >= 128: undefined behaviour in the reference -- is read as A as well and counted in
 * dbgk_stats.other_bytes), offsets[n_reads+1] = start of each read in `bases`, offsets[0] == 0.
 * HOST buffers; the call copies them through pinned double buffers and returns once the batch is
 * queued (asynchronous w.r.t. the device).  If `bases` is page-locked memory the GPU can read (hipHostMalloc,
 * hipHostRegister: detected with hipPointerGetAttributes) the sequences are copied host-to-device straight out of
 * it -- no staging copy, which is what bounds the pageable path -- and the call returns when the last of those
 * copies has run.  Either way the buffers may be reused on return.                                */
int dbgk_push_reads(dbgk_handle *h, const char *bases, const uint64_t *offsets, uint64_t n_reads);

/* the same without the copy: dbgk_push_acquire returns the handle's next pinned staging buffers -- room for cap_bases sequence
 * bytes and cap_reads + 1 offsets (offsets[0] = 0); it waits until the batch that used them last has left for the device -- the
 * caller fills them (a parser writes its reads there directly) and dbgk_push_commit(n_reads) queues the batch.  One acquire
 * per commit; dbgk_push_reads may be mixed in between batches.                                                        */
int dbgk_push_acquire(dbgk_handle *h, char **bases, uint64_t **offsets, uint64_t *cap_bases, uint64_t *cap_reads);
int dbgk_push_commit(dbgk_handle *h, uint64_t n_reads);

/* ---- 2-bit packed reads ------------------------------------------------------------------------
 * The reference's alphabet is two bits wide by definition (alphabet[], seqKmer.cpp:9-19: A a N n -> 0, C c -> 1, G g -> 2,
 * T t -> 3), so a reader can hand the reads over packed -- a quarter of the bytes over PCIe, and the level-1 kernels skip
 * their ASCII decode.  FORMAT: the bases of all reads back to back (no separators, like `bases` above), 16 per 32-bit word,
 * base i in bits 31 - 2 * (i % 16) .. 30 - 2 * (i % 16) of word i / 16 (first base in the top bits, as seq2bit packs a
 * k-mer, seqKmer.cpp:34-41); offsets[] count BASES, offsets[0] may be any base position of `packed`.
 * dbgk_pack_bases: the packer (host, any thread; AVX2 when the CPU has it): n_bases ASCII bytes -> bits of `packed` starting at
 *   base position first_base.  Bytes outside ACGTNacgtn become A and are counted: *other_bytes += their number.  Words that a
 *   call covers only partly (its first / last) are OR-ed into atomically, so several threads may pack neighbouring ranges of
 *   one buffer -- such boundary words must be zero beforehand.  dbgk_unpack_bases is its inverse (upper-case letters).
 * dbgk_push_reads_packed: dbgk_push_reads for such a buffer in HOST memory (page-locked memory is read by the copy engine
 *   directly); other_bytes = what the packer counted for these reads, added to dbgk_stats.other_bytes.
 * dbgk_push_commit_packed: commit for a batch that was written PACKED into the buffers of dbgk_push_acquire (the `bases`
 *   buffer taken as uint32_t words, offsets[0] = 0; a batch still holds at most cap_bases bases).
 * dbgk_push_reads_packed_device: the packed words and the offsets are in device memory (d_packed 16-byte aligned, readable
 *   through word (n_bases + 15) / 16 - 1); dbgk_pack_bases_device makes such a buffer from ASCII bases in device memory.
 * Every engine takes packed batches except DBGK_ENGINE_SEEDIDX, whose windows are cut at 'N' (DBGK_ERR_ARG).             */
int dbgk_pack_bases(const char *bases, uint64_t n_bases, uint32_t *packed, uint64_t first_base, uint64_t *other_bytes);
/* the same for n_reads sequences that lie anywhere in memory (a parser's view of a file window), packed back to back from base
 * position first_base on -- one call per reader thread and share of a batch; only the first and the last word of the call's range are
 * OR-ed into (zero beforehand where a neighbour shares them)                                                                   */
typedef struct dbgk_read_ref {
	const char *seq;
	uint32_t    len;
} dbgk_read_ref;
int dbgk_pack_reads(const dbgk_read_ref *reads, uint64_t n_reads, uint32_t *packed, uint64_t first_base, uint64_t *other_bytes);
int dbgk_unpack_bases(const uint32_t *packed, uint64_t first_base, uint64_t n_bases, char *bases);
int dbgk_push_reads_packed(dbgk_handle *h, const uint32_t *packed, const uint64_t *offsets, uint64_t n_reads, uint64_t other_bytes);
int dbgk_push_commit_packed(dbgk_handle *h, uint64_t n_reads, uint64_t other_bytes);
int dbgk_push_reads_packed_device(dbgk_handle *h, const uint32_t *d_packed, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases);
int dbgk_pack_bases_device(dbgk_handle *h, const char *d_bases, uint64_t n_bases, uint32_t *d_packed);
/* reads of ONE length (what a sequencer writes, before anything trims them): n_reads reads of read_len bases each, back to back in the
 * packed format.  No offsets travel (at 150 bases they are a sixth of the packed bytes) and no statistics pass runs in front of
 * level 1; engines that navigate by offsets get them made on the device.  Otherwise like dbgk_push_reads_packed[_device].      */
int dbgk_push_reads_packed_uniform(dbgk_handle *h, const uint32_t *packed, uint64_t n_reads, uint32_t read_len, uint64_t other_bytes);
int dbgk_push_reads_packed_uniform_device(dbgk_handle *h, const uint32_t *d_packed, uint64_t n_reads, uint32_t read_len);

/* same, for reads already resident in device memory of the handle's GPU (both pointers 16-byte
 * aligned, readable through the end of the last read).  Nothing is copied; the buffers must stay
 * valid until the next dbgk_sync/dbgk_finalize.                                                  */
int dbgk_push_reads_device(dbgk_handle *h, const char *d_bases, const uint64_t *d_offsets,
                           uint64_t n_reads, uint64_t n_bases);

/* replaces the tail of build_debruijn_graph (DBGgraph.cpp:418, add_node_to_kmerset
 * kmerSet.cpp:253-273): completes all queued work, appends the key-0 node, reduces the counters.
 * Returns DBGK_ERR_TABLE_FULL if any insert ran out of slots.                                    */
int dbgk_finalize(dbgk_handle *h, dbgk_stats *out);

/* wait for all queued work of the handle */
int dbgk_sync(dbgk_handle *h);

/* replaces enlarge_kmerset_parallel (kmerSet.cpp:132-189) for the DEVICE table: allocates a table
 * of new_slots, re-seats every node, frees the old one.  Content (the node multiset) is unchanged.
 * Allowed between pushes (it synchronises first; a PARTITION handle flushes its records first and
 * re-plans its bucket geometry for the new size, which must again be in the engine's range).      */
int dbgk_resize_table(dbgk_handle *h, uint64_t new_slots);

/* PARTITION engine, input of unknown size (the block loop of parse_one_reads_file, DBGgraph.cpp:226-356,
 * never knows how much is still to come): turn the records pushed so far into table nodes NOW.  Regions
 * that already hold nodes of an earlier flush are loaded back into LDS, the new records inserted, the
 * region written out again; the record store is empty afterwards and dbgk_refresh_stats is exact (between
 * flushes its counts exclude what still sits in the store).  Pushes do this on their own when the store
 * is full.  No-op for the other engines (their table is always current).                           */
int dbgk_flush(dbgk_handle *h);
/* PARTITION engine: upper bound of the k-mer occurrences waiting in the record store, and what the
 * store was sized for (0, 0 for the other engines)                                                 */
int dbgk_store_room(dbgk_handle *h, uint64_t *pending_kmers, uint64_t *capacity_kmers);

/* ---- results ----------------------------------------------------------------------------------- */

/* fills a host KmerSet: `array` (host_size nodes) and `nul_flag` (host_size/8+1 bytes, bit i =
 * byte i/8 mask 128>>(i%8), kmerSet.cpp:53) such that every key is reachable by linear probing
 * from hash_code(key) % host_size without crossing a clear flag (exist_kmerset kmerSet.cpp:280-302),
 * unused slots are all-zero, and the key-0 node sits on key 0's probe chain.  host_size may differ
 * from table_slots (the table is then re-seated on the device first: the GPU counterpart of
 * enlarge_kmerset_parallel, kmerSet.cpp:132-189).  Every slot of `array` and every byte of `nul_flag`
 * is written (the buffers need not be zeroed; ordinary pageable memory).  Tables of 256 MiB and more
 * cross the link as their occupied nodes + the occupancy bits and are laid out at their slots by host
 * threads (DBGK_EXPORT_THREADS, default 12), through the handle's idle page-locked batch buffers
 * where it has them: same bytes, a third of the traffic at the reference's load factors.           */
int dbgk_export_host_table(dbgk_handle *h, uint64_t host_size, dbgk_node *array, uint8_t *nul_flag);

/* dbgk_export_host_table + the WHOLE first pass of the consumer, calculate_kmer_links (DBG_contig/contig.cpp:107-181), computed
 * on the device for exactly the table that is handed over, so that the consumer can skip its serial scan of it:
 *   klink[host_size]      the 2-byte KmerLink record of every slot (contig.h:31-42): byte 0 = l_link_num | l_link_base << 2 |
 *                         r_link_num << 4 | r_link_base << 6, byte 1 bit 0 = linear; 0 for empty slots (the consumer zeroes klink,
 *                         contig.cpp:60).  link number = counters > kmer_freq_cutoff, at most 3; base = first base with the
 *                         largest such counter (contig.cpp:129-163)
 *   del_flag[host_size/8+1]  bit set (128 >> (i % 8) of byte i / 8, kmerSet.h:161-164) for nodes with no link above the cutoff
 *                         (contig.cpp:165-168); all other bits 0
 *   tip_nodes / branch_nodes  slots with l_link_num + r_link_num == 1 / with a side of more than one link, in ASCENDING slot
 *                         order -- the order of the reference's loop (contig.cpp:119,173-178); either may be NULL (counts only);
 *                         *n_tips / *n_branches always return the counts; DBGK_ERR_CAPACITY when a list does not fit
 *   stats                 DepthStat[256] and the five class counts (optional)
 * Unsharded handles.  PARITY UNPINNED: contig.cpp needs Boost headers, absent here, so this is checked against this build's
 * restatement of those lines (tests), not against the compiled reference.                                                       */
int dbgk_export_host_table_links(dbgk_handle *h, uint64_t host_size, dbgk_node *array, uint8_t *nul_flag, int32_t kmer_freq_cutoff,
                                 uint16_t *klink, uint8_t *del_flag, uint64_t *tip_nodes, uint64_t tip_capacity, uint64_t *n_tips,
                                 uint64_t *branch_nodes, uint64_t branch_capacity, uint64_t *n_branches, dbgk_link_stats *stats);

/* canonical dump: all nodes sorted by kmer (the parity artefact of SURVEY.md section 8(a)).
 * `capacity` = number of nodes `out` can hold (>= stats.count).                                  */
int dbgk_export_sorted(dbgk_handle *h, dbgk_node *out, uint64_t capacity, uint64_t *n_out);

/* all non-zero-key nodes sorted by the position of their first occurrence (needs
 * DBGK_FLAG_TRACK_FIRST_SEEN): out[i] and first_pos[i] (index into the concatenation of everything
 * pushed) for i < *n_out.  Replaying out[] through the reference's sequential insert and enlarge
 * schedule reproduces its -t 1 slot layout (host side: DBGK_LAYOUT=ref).   */
int dbgk_export_first_seen_order(dbgk_handle *h, dbgk_node *out, uint64_t *first_pos, uint64_t capacity, uint64_t *n_out);

/* order-independent digest of the node multiset: sum over nodes of
 * mix64(kmer ^ mix64((l_link << 32) | r_link)) mod 2^64, mix64 = splitmix64 finaliser             */
int dbgk_digest(dbgk_handle *h, uint64_t *digest);

/* calculate_kmer_links first pass (contig.cpp:119-181) on the device table                      */
int dbgk_link_stats_device(dbgk_handle *h, int32_t kmer_freq_cutoff, dbgk_link_stats *out);

/* ---- WIDE engine (k <= 63, 128-bit keys): results as 32-byte nodes, include/dbgk_wide.h ------------
 * canonical dump sorted by (kmer_hi, kmer_lo), the key-0 node first; `capacity` >= stats.count             */
int dbgk_wide_export_sorted(dbgk_handle *h, dbgk_node32 *out, uint64_t capacity, uint64_t *n_out);
/* host-layout table of host_size == table_slots nodes + nul_flag (bit i = byte i/8, mask 128 >> (i%8)): every key
 * reachable by linear probing from hash128(key) % host_size without crossing a clear flag, unused slots all-zero,
 * the key-0 node on key 0's chain -- the invariants of SURVEY 8(b) with the 128-bit hash                      */
int dbgk_wide_export_host_table(dbgk_handle *h, uint64_t host_size, dbgk_node32 *array, uint8_t *nul_flag);
/* dbgk_wide_export_host_table + the consumer's whole first pass for that table: dbgk_export_host_table_links for 32-byte nodes.
 * Same arguments, optional outputs, DBGK_ERR_CAPACITY and result layout; host_size == table_slots.  The pass reads the device
 * table in place; the nodes the host puts on their chains afterwards (zero low word, key 0) are added on the host.  Unsharded
 * WIDE handles (others: DBGK_ERR_STATE).  PARITY UNPINNED above k = 32.  (ABI 7, appended)                                     */
int dbgk_wide_export_host_table_links(dbgk_handle *h, uint64_t host_size, dbgk_node32 *array, uint8_t *nul_flag, int32_t kmer_freq_cutoff,
                                      uint16_t *klink, uint8_t *del_flag, uint64_t *tip_nodes, uint64_t tip_capacity, uint64_t *n_tips,
                                      uint64_t *branch_nodes, uint64_t branch_capacity, uint64_t *n_branches, dbgk_link_stats *stats);
/* several GPUs: every GPU builds the graph of its share of the reads (reads shard by record), then ships each node to
 * its owner, (hash128(key) >> 32) % n_parts -- the device analogue of the reference's `kmer % threadNum` ownership
 * (DBGgraph.cpp:148) -- which adds the counters up (per-byte saturating, exact for any split of the input).
 * dbgk_wide_partition_export: counts[p] = nodes owned by part p (this handle's key-0 node counts for part 0); with
 * d_nodes != NULL the nodes are written grouped by owner into that DEVICE buffer (part p at sum(counts[0..p))).
 * dbgk_wide_merge_nodes: insert-if-absent / saturating add of n nodes held in device memory of the handle's GPU;
 * allowed before and after dbgk_finalize (dbgk_refresh_stats recounts).                                        */
int dbgk_wide_partition_export(dbgk_handle *h, uint32_t n_parts, dbgk_node32 *d_nodes, uint64_t capacity, uint64_t *counts);
int dbgk_wide_merge_nodes(dbgk_handle *h, const dbgk_node32 *d_nodes, uint64_t n);
/* WIDE through records, SHARDS and PASSES.  shard_count = N: N handles (one per GPU) hold ONE table of table_slots slots, rank d
 * the slot range of its level-1 buckets -- the device analogue of the reference's `kmer % threadNum` ownership
 * (DBGgraph.cpp:148), as for 64-bit keys; the protocol is dbgk_shard_buffers / _mark_exchanged / _plan / _build_range /
 * _outgoing / _overflow / _merge below, with 16-byte records and 32-byte list entries (dbgk_node32: nodes {hi, lo, l_link, r_link},
 * observations {hi, lo, lb, rb}).  Keys whose low word is 0 and the key-0 node live outside the table (a 4096-slot side table per
 * handle): after dbgk_finalize they are gathered onto shard 0 -- dbgk_shard_side_export on every other shard (device list, the
 * key-0 node first), dbgk_wide_merge_nodes of that list on shard 0, dbgk_shard_side_clear on the others.
 * PASSES: the level-1 kernel fans out to at most 1024 buckets (counted over all shards) and a pass's records must fit the device,
 * so a big job reads its input n_passes times, the way disk-based k-mer counters pass over their input once per set of
 * partitions: for p in 0 .. n_passes-1 { dbgk_wide_begin_pass(p); push ALL reads; [exchange the buffers of dbgk_shard_buffers,
 * dbgk_shard_mark_exchanged;] dbgk_wide_end_pass } then dbgk_finalize.  Pass p keeps the records of own-bucket indices
 * [p * Bp, (p+1) * Bp) of every shard and completes those regions of the table; totals count the input once.  A handle with one
 * shard and one pass needs none of these calls.                                                                           */
int dbgk_wide_pass_info(dbgk_handle *h, uint32_t *n_passes, uint32_t *passes_done);
int dbgk_wide_begin_pass(dbgk_handle *h, uint32_t pass);
int dbgk_wide_end_pass(dbgk_handle *h);
int dbgk_shard_side_export(dbgk_handle *h, dbgk_node32 **d_nodes, uint64_t *n);
int dbgk_shard_side_clear(dbgk_handle *h);

/* ---- KFREQ engine: the k-mer frequency table of the correct_error module --------
 * The reference only CONSUMES this table (its producer, `kmerfreq`, is not part of the repository):
 * 8-bit format = 4^k saturating counts indexed by k-mer value, read by
 * correct_error/main.cpp:161-220; 1-bit format = bitmap, bit 128 >> (v % 8) of byte v / 8, read by
 * correct_error/main_parallel_senior.cpp:334-408 which mirrors bit v to its reverse complement only
 * when v <= rc(v) -- so counts live on the canonical (smaller) k-mer.  push_reads / finalize work as
 * for the graph engines; stats.count = number of distinct canonical k-mers.                       */
int dbgk_kfreq_export_counts(dbgk_handle *h, uint64_t first_kmer, uint64_t n, uint8_t *host_out);
/* n_bytes bytes of the bit table starting at byte first_byte: bit set when count > cutoff          */
int dbgk_kfreq_export_bits(dbgk_handle *h, uint32_t cutoff, uint64_t first_byte, uint64_t n_bytes, uint8_t *host_out);
/* Partial tables of several GPUs: counts[first_kmer, first_kmer + n) of a finalized handle
 * += n counters held in device memory of the handle's GPU, per-byte saturating -- exact, because
 * min(255, min(255,a) + min(255,b)) = min(255, a+b).  first_kmer, n and the address: multiples of 16.
 * dbgk_kfreq_device_counts: the handle's 4^k counters in device memory (what a peer sends).          */
int dbgk_kfreq_merge_counts(dbgk_handle *h, const uint8_t *d_counts, uint64_t first_kmer, uint64_t n);
int dbgk_kfreq_device_counts(dbgk_handle *h, uint8_t **d_counts, uint64_t *n);
/* The k-mer frequency spectrum, computed on the device (additions to ABI 7): hist[c] = number of k-mer values v in
 * [first_kmer, first_kmer + n) whose counter equals c (c = 255: 255 or more); the 256 bins sum to n.  Any first_kmer
 * and n inside 4^k; errors as for dbgk_kfreq_export_counts.                                                       */
int dbgk_kfreq_spectrum(dbgk_handle *h, uint64_t first_kmer, uint64_t n, uint64_t hist[256]);
/* device time in ms of the histogram kernel of the handle's last dbgk_kfreq_spectrum (0 before the first, and for n = 0) */
int dbgk_kfreq_spectrum_ms(dbgk_handle *h, double *ms);

/* ---- SEEDIDX engine: the contig k-mer index of the link_scaffold module ----------
 * chop_contig_to_kmerset (link_scaffold/map_func.cpp:119-173): push the contig sequences with
 * dbgk_push_reads (contig index = order of pushing; windows never span an upper-case 'N'), finalize,
 * export.  Nodes come out as the reference's 16-byte KmerNode of THAT module
 * (link_scaffold/kmerSet.h:54-61): kmer, then one 64-bit word {id:32, pos:30, freq:1, direct:1}
 * (low bits first) -- held in dbgk_node as l_link = low dword, r_link = high dword.  Key 0 is an
 * ordinary key here (the reference tests emptiness with nul_flag, not kmer == 0).
 * dbgk_seed_export_host_table fills a table every key of which is reachable from
 * hash_code(key) % host_size without crossing a clear nul_flag bit (exist_kmerset,
 * link_scaffold/kmerSet.cpp:216-238).                                                              */
int dbgk_seed_export_sorted(dbgk_handle *h, dbgk_node *out, uint64_t capacity, uint64_t *n_out);
int dbgk_seed_export_host_table(dbgk_handle *h, uint64_t host_size, dbgk_node *array, uint8_t *nul_flag);

/* ---- phase A alone (parity of the extraction kernel) ------------------------------------------ */

/* thread_parseBlock only (DBGgraph.cpp:38-120) on host buffers: for every base position p of
 * `bases` writes valid[p] (1 if a k-mer window starts at p inside its read after trimming), and
 * for valid positions kmer[p], left[p], right[p] exactly as StoreKmer/StoreLeftBase/StoreRightBase
 * would hold them for (read i, j = p - offsets[i]).  All four outputs are HOST arrays of
 * offsets[n_reads] entries.                                                                      */
int dbgk_extract_kmers(dbgk_handle *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                       uint64_t *kmer, uint8_t *left, uint8_t *right, uint8_t *valid);

/* ---- multi-GPU building blocks (reads shard by record, keys are owned by hash) ---------------- */

/* owner of a key among n_parts ranks: (hash_code(key) >> 32) % n_parts -- the device analogue of
 * the reference's `kmer % threadNum` ownership (DBGgraph.cpp:148).  After dbgk_finalize:
 * counts[p] = number of nodes of this handle's table owned by part p (host array, n_parts).      */
int dbgk_partition_counts(dbgk_handle *h, uint32_t n_parts, uint64_t *counts);
/* writes the nodes grouped by owner into the DEVICE buffer d_nodes (capacity nodes): part p
 * occupies [sum(counts[0..p)), +counts[p]).  The key-0 node is owned by part 0.                  */
int dbgk_partition_export(dbgk_handle *h, uint32_t n_parts, dbgk_node *d_nodes, uint64_t capacity);
/* merges n already-aggregated nodes (DEVICE buffer) into the table: insert-if-absent, otherwise
 * per-byte saturating add min(255, a+b) -- exact for any split of the input because
 * min(255, min(255,a)+min(255,b)) == min(255,a+b).  Allowed before and after dbgk_finalize; a
 * key-0 node in the input is folded into the handle's key-0 node.                                */
int dbgk_merge_nodes(dbgk_handle *h, const dbgk_node *d_nodes, uint64_t n);
/* recount after merges (finalize semantics without re-appending the key-0 node twice); also
 * usable between pushes to watch the load of the table                                          */
int dbgk_refresh_stats(dbgk_handle *h, dbgk_stats *out);
/* single-process multi-GPU: copy n nodes from a device buffer of src's GPU into a device buffer
 * of dst's GPU (peer copy over xGMI), synchronous                                               */
int dbgk_copy_nodes_peer(dbgk_handle *dst, dbgk_node *d_dst, dbgk_handle *src, const dbgk_node *d_src, uint64_t n);

/* ---- sharded table: reads shard by record, k-mers are owned by SLOT RANGE ---------------------
 * With shard_count = N every handle extracts its own reads into level-1 buckets of the GLOBAL table
 * (slot >> r); rank d owns the bucket range [d*B, (d+1)*B).  All N handles of a job must be created
 * with the same kmer_size, table_slots and expected_kmers (they fix the bucket geometry and the
 * capacity of the exchanged buffers; compare chunk_bytes across ranks if in doubt).  Between the pushes and dbgk_finalize
 * the caller moves chunk d of every rank's send buffer to rank d (an all-to-all: RCCL
 * ncclSend/ncclRecv, torch all_to_all_single, or peer copies), the bucket fill counts likewise,
 * then calls dbgk_shard_mark_exchanged.  finalize builds only the handle's slot range; the few
 * nodes whose probe runs off the end of a shard (dbgk_shard_outgoing) are handed to the next rank
 * (dbgk_shard_merge(..., from_previous_shard = 1)), bucket-overflow records (dbgk_shard_overflow,
 * normally none) are offered to every rank, which keeps its own.  Exact for the same reason the
 * reference's per-thread ownership is (DBGgraph.cpp:148): a key has exactly one home slot.       */
typedef struct dbgk_shard_info {
	uint32_t n_ranks, rank;
	uint64_t table_slots_global;
	uint64_t slot_lo, slot_hi;     /* this handle's slot range                                     */
	void    *d_send;               /* n_ranks chunks of chunk_bytes: chunk d goes to rank d        */
	void    *d_recv;               /* n_ranks chunks of chunk_bytes: chunk s comes from rank s     */
	uint64_t chunk_bytes;
	void    *d_send_cnt;           /* n_ranks chunks of cnt_chunk_bytes (u32 fill counts)          */
	void    *d_recv_cnt;
	uint64_t cnt_chunk_bytes;
	/* a chunk is buckets_per_rank level-1 buckets of bucket_bytes each (fill counts: cnt_bucket_bytes);
	 * this handle owns the first own_buckets of its range (the last rank may own fewer)          */
	uint32_t buckets_per_rank, own_buckets;
	uint64_t bucket_bytes, cnt_bucket_bytes;
} dbgk_shard_info;

/* The geometry a PARTITION handle of these parameters would get -- level-1 bucket width, fan-outs, this shard's slot range and
 * buckets, the bytes of its table shard and record stores -- WITHOUT touching a device (ABI 6): what a multi-GPU launcher plans
 * with before any rank has created its handle (bench.py --plan-only, tests/test_multigpu_gloo.py).  shard_count 0 = one
 * unsharded handle.  DBGK_ERR_ARG when the engine cannot take the table (2^26 <= table_slots < 2^34).                        */
typedef struct dbgk_plan_info {
	uint64_t table_slots;          /* the (global) table                                                       */
	uint32_t r;                    /* level-1 bucket = slot >> r                                               */
	uint32_t level1_buckets;       /* of the global table                                                      */
	uint32_t final_per_level1;     /* 4096-slot regions per level-1 bucket = level-2 fan-out                   */
	uint32_t three_level;          /* 1: level 2 runs as two passes (tables of 2^33 slots and more)            */
	uint32_t buckets_per_rank, own_buckets, first_bucket;
	uint32_t reserved;
	uint64_t slot_lo, slot_hi;     /* this shard's slot range                                                  */
	uint64_t records_per_level1_bucket, records_per_final_bucket; /* capacities                               */
	uint64_t table_bytes, level1_store_bytes, inbox_bytes, final_store_bytes; /* device memory of this shard   */
} dbgk_plan_info;
int dbgk_plan_partition(uint64_t table_slots, uint64_t expected_kmers, uint32_t shard_count, uint32_t shard_index, dbgk_plan_info *out);

int dbgk_shard_buffers(dbgk_handle *h, dbgk_shard_info *out);
int dbgk_shard_mark_exchanged(dbgk_handle *h);
/* Exchange and build IN PIECES, so that the transfer of later buckets overlaps the build of earlier
 * ones: once the fill counts have been exchanged call dbgk_shard_plan; whenever the records of the
 * own buckets [j0, j1) have arrived from every rank (bucket j of chunk s of d_recv) call
 * dbgk_shard_build_range(j0, j1) -- ranges in ascending order, each bucket once; the kernels are
 * queued on the handle's streams and the call returns.  dbgk_shard_mark_exchanged + dbgk_finalize
 * then build whatever is left and complete the step.                                            */
int dbgk_shard_plan(dbgk_handle *h);
int dbgk_shard_build_range(dbgk_handle *h, uint32_t j0, uint32_t j1);
/* after dbgk_finalize: device list of nodes that left this shard / of overflow observations
 * {kmer, lb | rb << 8}; the lists stay valid until the next dbgk_reset                            */
int dbgk_shard_outgoing(dbgk_handle *h, dbgk_node **d_nodes, uint64_t *n);
int dbgk_shard_overflow(dbgk_handle *h, dbgk_node **d_triples, uint64_t *n);
/* once the overflow list is full, further observations are aggregated in a side table of n_slots nodes
 * (empty slots are all-zero); n_slots = 0 when it was not needed.  Like the overflow list it may hold keys
 * of any shard: offer it to every rank with dbgk_shard_merge(..., is_triple = 0, from_previous_shard = 0)   */
int dbgk_shard_heavy(dbgk_handle *h, dbgk_node **d_table, uint64_t *n_slots);
/* merge nodes (is_triple = 0) or observations (is_triple = 1) held in device memory of this GPU:
 * entries whose home slot lies in another shard are ignored unless from_previous_shard is set,
 * in which case they continue their probe at this shard's first slot                            */
int dbgk_shard_merge(dbgk_handle *h, const dbgk_node *d_nodes, uint64_t n, int is_triple, int from_previous_shard);
/* fold another handle's key-0 node into this one (per-byte saturating add)                      */
int dbgk_add_polyA(dbgk_handle *h, uint32_t l_link, uint32_t r_link);
int dbgk_memcpy_d2d(dbgk_handle *h, void *d_dst, const void *d_src, size_t bytes);

/* ---- several GPUs inside one process (the C++ host layer with DBGK_GPUS=N) ------------------------
 * A communicator owns n sharded handles of ONE table of cfg->table_slots slots (shard i on devices[i]; the
 * same device may appear more than once -- n shards on one GPU, which is how the tests exercise the path).
 * cfg->expected_kmers sizes the record store of EACH handle; engine, shard_count and shard_index of cfg are
 * set by the call.  Reads shard by record (dbgk_comm_push_reads deals batches round robin), k-mers are owned
 * by slot range -- the device analogue of the reference's `kmer % threadNum` ownership
 * (DBG_contig/DBGgraph.cpp:148).  flush / finalize move every level-1 record bucket to its owner with peer
 * copies over xGMI (hipMemcpyPeerAsync, in pieces that overlap the region build of the previous piece), build
 * each shard's slot range and hand over the few stragglers (overflow observations, nodes that probed past the
 * end of a shard).  Same protocol as the one-process-per-GPU flow over RCCL (dbg_assembly_amd/multigpu.py).
 * One host thread per communicator.                                                                 */
typedef struct dbgk_comm dbgk_comm;
int dbgk_comm_create(const dbgk_config *cfg, const int32_t *devices, uint32_t n, dbgk_comm **out);
int dbgk_comm_destroy(dbgk_comm *c);
uint32_t dbgk_comm_size(const dbgk_comm *c);
dbgk_handle *dbgk_comm_handle(dbgk_comm *c, uint32_t i);
int dbgk_comm_push_reads(dbgk_comm *c, const char *bases, const uint64_t *offsets, uint64_t n_reads);
int dbgk_comm_push_reads_packed(dbgk_comm *c, const uint32_t *packed, const uint64_t *offsets, uint64_t n_reads, uint64_t other_bytes);
/* records -> table on every shard now (dbgk_flush for a communicator); a push does it when a store is full */
int dbgk_comm_flush(dbgk_comm *c);
/* enlarge_kmerset_parallel (kmerSet.cpp:132-189) for the table of a communicator: flushes, creates shards of a table of new_slots
 * slots, re-seats every node into the shard that owns its new home slot, frees the old shards.  The node multiset and the totals
 * are unchanged; handles obtained from dbgk_comm_handle before the call are gone.  Graph communicators only.                  */
int dbgk_comm_resize(dbgk_comm *c, uint64_t new_slots);
/* totals of the whole job (count includes the one key-0 node); exact after a flush                       */
int dbgk_comm_refresh_stats(dbgk_comm *c, dbgk_stats *out);
int dbgk_comm_finalize(dbgk_comm *c, dbgk_stats *out);
int dbgk_comm_digest(dbgk_comm *c, uint64_t *digest);
int dbgk_comm_link_stats(dbgk_comm *c, int32_t kmer_freq_cutoff, dbgk_link_stats *out);
/* the host KmerSet of the whole job (same contract as dbgk_export_host_table): the shards side by side when
 * host_size is the global table size, otherwise every node re-seated on the host                          */
int dbgk_comm_export_host_table(dbgk_comm *c, uint64_t host_size, dbgk_node *array, uint8_t *nul_flag);
/* dbgk_export_host_table_links for a communicator: the host table of the whole job AND the consumer's first pass for it (klink,
 * del_flag, the ascending tip / branch slot lists, DepthStat: contig.cpp:107-181), computed on the device.  The shards' nodes are
 * first assembled in one table of host_size slots on the first member's device (host_size * 16 bytes must be free there).  Same
 * arguments, results and (un)pinned parity as dbgk_export_host_table_links.                                                  */
int dbgk_comm_export_host_table_links(dbgk_comm *c, uint64_t host_size, dbgk_node *array, uint8_t *nul_flag, int32_t kmer_freq_cutoff,
                                      uint16_t *klink, uint8_t *del_flag, uint64_t *tip_nodes, uint64_t tip_capacity, uint64_t *n_tips,
                                      uint64_t *branch_nodes, uint64_t branch_capacity, uint64_t *n_branches, dbgk_link_stats *stats);
/* cfg->engine == DBGK_ENGINE_WIDE (k <= 63, expected_kmers > 0 = what EACH member extracts): n slot-range shards of one table of
 * 32-byte nodes; the reads stream through once (a geometry that needs several passes is refused: drive the handles yourself with
 * dbgk_wide_begin_pass), the record stores are built at dbgk_comm_finalize.  Results of the whole job:                          */
int dbgk_comm_wide_export_sorted(dbgk_comm *c, dbgk_node32 *out, uint64_t capacity, uint64_t *n_out);
int dbgk_comm_wide_export_host_table(dbgk_comm *c, uint64_t host_size, dbgk_node32 *array, uint8_t *nul_flag);
/* dbgk_wide_export_host_table_links for the shards of one table: the pass runs per shard on its slot range, slot numbers are those
 * of the whole table, lists ascending over all shards.  (ABI 7, appended)                                                       */
int dbgk_comm_wide_export_host_table_links(dbgk_comm *c, uint64_t host_size, dbgk_node32 *array, uint8_t *nul_flag, int32_t kmer_freq_cutoff,
                                           uint16_t *klink, uint8_t *del_flag, uint64_t *tip_nodes, uint64_t tip_capacity, uint64_t *n_tips,
                                           uint64_t *branch_nodes, uint64_t branch_capacity, uint64_t *n_branches, dbgk_link_stats *stats);
/* cfg->engine == DBGK_ENGINE_KFREQ: a communicator of n whole frequency tables.  Every member counts the reads
 * dealt to it; dbgk_comm_finalize makes member d the owner of an n-th of the k-mer values and adds the other
 * members' slices of that range to its own (peer copies in chunks, overlapped with the saturating add).  The
 * two exports read every range from its owner; stats.count = distinct canonical k-mers of the whole job.     */
int dbgk_comm_kfreq_export_counts(dbgk_comm *c, uint64_t first_kmer, uint64_t n, uint8_t *host_out);
int dbgk_comm_kfreq_export_bits(dbgk_comm *c, uint32_t cutoff, uint64_t first_byte, uint64_t n_bytes, uint8_t *host_out);
/* dbgk_kfreq_spectrum of the whole table: every member over the range it owns, summed (additions to ABI 7) */
int dbgk_comm_kfreq_spectrum(dbgk_comm *c, uint64_t hist[256]);

/* ---- utilities --------------------------------------------------------------------------------- */

/* synthetic reads (include/dbgk_synth.h) generated straight into device memory: d_bases gets
 * n_reads * read_len bytes, d_offsets n_reads+1 entries                                          */
int dbgk_synth_reads_device(dbgk_handle *h, const dbgk_synth_params *p, uint64_t first_read,
                            uint64_t n_reads, char *d_bases, uint64_t *d_offsets);

int dbgk_device_malloc(dbgk_handle *h, size_t bytes, void **d_ptr);
int dbgk_device_free(dbgk_handle *h, void *d_ptr);
int dbgk_memcpy_d2h(dbgk_handle *h, void *dst, const void *d_src, size_t bytes);
int dbgk_memcpy_h2d(dbgk_handle *h, void *d_dst, const void *src, size_t bytes);

int dbgk_get_timings(dbgk_handle *h, dbgk_timings *out);
int dbgk_reset_timings(dbgk_handle *h);
/* HIP stream of the handle as an opaque pointer (hipStream_t), for callers that time with events */
void *dbgk_stream(dbgk_handle *h);

/* the measured-HBM denominator of the roofline (GB/s, bytes read + bytes written): the best of the runtime's device-to-device
 * memcpy and this library's own streaming copy kernels (16 bytes per lane, default and non-temporal policy, 1 and 2 workgroups
 * per CU) over two buffers of `bytes` each (use >= 2 GiB: far beyond the 256 MiB Infinity Cache), `iters` copies per variant   */
int dbgk_measure_copy_bandwidth(dbgk_handle *h, size_t bytes, int iters, double *gbps);
/* the same, and the runtime's hipMemcpyDtoD figure alone next to the best (ABI 6): bench.py reports both denominators */
int dbgk_measure_copy_bandwidth2(dbgk_handle *h, size_t bytes, int iters, double *gbps, double *runtime_memcpy_gbps);
/* random 64-byte gather over a buffer of `bytes` (the practical random-access ceiling of the engines
 * that touch one random node per k-mer occurrence): n_accesses sectors fetched, GB/s and G sectors/s             */
int dbgk_measure_gather_bandwidth(dbgk_handle *h, size_t bytes, uint64_t n_accesses, double *gbps, double *gaccesses_per_s);

/* ---- CORRECT: correct_error_reads on the GPU (ABI 7) ------------------------------------------------------------------
 * The reference's correct_error_reads (correct_error/main_parallel_senior.cpp + correct.cpp): every read is corrected
 * against the loaded 1-bit k-mer table, output identical to the reference's for the same table, reads and options.
 * The table is built on the device either from the raw bits of a 1-bit .cz file (dbgk_corr_load_bits, then
 * dbgk_corr_seal applies the loader's mirror: bit v -> rc(v) when v <= rc(v)) or from a finalized KFREQ handle
 * (dbgk_corr_from_kfreq: bit(v) = count[canonical(v)] > cutoff, what kmerfreq -b 1 -m cutoff writes, loaded).   */
typedef struct dbgk_corr dbgk_corr;

typedef struct dbgk_corr_params {
	int32_t k;                  /* -k, 1..19 (4^19 bits = 32 GiB); 1..18 for dbgk_corr_from_kfreq                     */
	int32_t min_high_region;    /* -m HighFreqRegLenCutoff, >= 1 (the reference's default is 17 whatever -k is)     */
	int32_t max_change;         /* -c Max_change_in_one_read, >= 0 (default 2)                                      */
	int32_t further_trim;       /* -x Further_trim_len, >= 0 (default 17 whatever -k is)                            */
	int32_t max_tree_nodes;     /* -n Max_node_in_BB_tree, 1 .. 2^26 - 1 (TreeNode.pointer is 26 bits; default 5000000) */
	int32_t min_trimmed_len;    /* -r Min_trimmed_read_len, >= 0 (default 75)                                       */
} dbgk_corr_params;

/* per read */
typedef struct dbgk_corr_rec {
	uint32_t one_base;          /* bases changed by the one-base fix (correct_one_base)                             */
	uint32_t tree;              /* bases changed by the branch-and-bound trees                                      */
	uint32_t left_trim;         /* LeftEndTrim / RightEndTrim as the reference prints them                          */
	uint32_t right_trim;
	uint32_t node_limit_hits;   /* trees that reached -n ("node_vec_pos exceed Max_node_in_BB_tree")              */
	uint8_t deleted;            /* IsDeleted                                                                        */
	uint8_t path;               /* finished by 0: the classify kernel, 1: the correct kernel, 2: the overflow kernel */
	uint8_t pad[2];
} dbgk_corr_rec;

typedef struct dbgk_corr_stats {
	uint64_t reads;
	uint64_t by_classify;       /* reads whose k-mers were all high (or that have none)                             */
	uint64_t by_correct;        /* reads corrected with read, mask and tree frontier in LDS                         */
	uint64_t by_overflow;       /* reads whose frontier or length did not fit in LDS                                */
	uint64_t node_limit_hits;
	double ms_classify, ms_correct, ms_overflow;  /* device time of each kernel of the last batch                  */
} dbgk_corr_stats;

/* DBGK_ERR_ARG on a bad parameter, before any device work */
int dbgk_corr_create(const dbgk_corr_params *p, int device, dbgk_corr **out);
int dbgk_corr_destroy(dbgk_corr *c);
/* n_bytes raw bytes of the file's table (its decompressed blocks) at byte first_byte; then seal once */
int dbgk_corr_load_bits(dbgk_corr *c, uint64_t first_byte, uint64_t n_bytes, const uint8_t *host_bits);
int dbgk_corr_seal(dbgk_corr *c);
int dbgk_corr_from_kfreq(dbgk_corr *c, dbgk_handle *kfreq, uint32_t cutoff);
/* Kmer_theory_total (4^k) and Kmer_hifreq_num of the loader */
int dbgk_corr_table_stats(dbgk_corr *c, uint64_t *theory_total, uint64_t *hifreq);
/* n_bytes bytes of the loaded table at byte first_byte (bit v: byte v / 8, bit 128 >> v % 8) */
int dbgk_corr_export_bits(dbgk_corr *c, uint64_t first_byte, uint64_t n_bytes, uint8_t *host_out);
/* n reads, read i = seq[offsets[i], offsets[i+1]) (offsets[0] == 0, each read < 2^29 bytes).  out_seq (offsets[n]
 * bytes): every read after correction, untrimmed, at its input offset; out_rec: n records.  Input order is kept. */
int dbgk_corr_reads(dbgk_corr *c, const char *seq, const uint64_t *offsets, uint64_t n, char *out_seq, dbgk_corr_rec *out_rec);
int dbgk_corr_batch_stats(dbgk_corr *c, dbgk_corr_stats *out);
/* simulate_lowfreq_kmer's scan (correct_error/simulate_lowfreq_kmer.cpp:71-119; additions to ABI 7) against the loaded
 * table, which must be marked on both strands as every table of this section is.  Sequence i = seq[offsets[i],
 * offsets[i+1]) (offsets[0] == 0, any length).  Site t of a sequence of L >= 2k - 1 bases is the fragment
 * seq[t * skip, t * skip + 2k - 1) for every t * skip <= L - (2k - 1); its middle base becomes (code + 1) mod 4
 * (ACGT = 0..3 in either case, N and any other byte = 0) and hist[number of its k windows absent from the table]++.
 * hist (k + 1 entries) is overwritten.  skip == 0: DBGK_ERR_ARG.  dbgk_corr_batch_stats is left as it was.          */
int dbgk_corr_mutation_scan(dbgk_corr *c, const char *seq, const uint64_t *offsets, uint64_t n_seqs, uint32_t skip, uint64_t *hist);
/* device time in ms of the scan kernel of the last dbgk_corr_mutation_scan (0 before the first, and for a scan without sites) */
int dbgk_corr_mutation_scan_ms(dbgk_corr *c, double *ms);

/* The corrected reads stay on the device (additions to ABI 7).  The COMPACT batch is what the command line writes as sequence
 * lines, without the text: read i trimmed to deleted ? 0 : L - left_trim - right_trim bytes from byte left_trim on (a record
 * that trims more than its read holds -- the kernels write none for a read they keep -- gives 0), the reads back to back in
 * input order, a deleted read of length 0 at its place (offsets[i + 1] == offsets[i], so pairs stay pairs).  On the device the
 * bases start on a 16-byte boundary and fill whole 16-byte vectors, the pad of the last one 0; the offsets are n + 1 64-bit
 * values.  The gather kernel works in tiles of DBGK_CORR_COMPACT_TILE output bytes.                                         */
#define DBGK_CORR_COMPACT_TILE 4096
typedef struct dbgk_corr_compact_info {
	uint64_t reads;             /* reads of the batch, deleted ones included                                        */
	uint64_t result_reads;      /* num_result_reads / num_result_bases of <file>.correct.stat                       */
	uint64_t result_bases;
	uint64_t trimmed_reads;     /* num_trimmed_reads / num_trimmed_bases (kept reads only)                          */
	uint64_t trimmed_bases;
	uint64_t deleted_reads;
	uint64_t one_base;          /* num_corrected_bases_by_Fast_method / _by_BBtree_method (kept reads only)         */
	uint64_t tree;
	uint64_t node_limit_hits;   /* as dbgk_corr_stats: all reads                                                    */
	uint64_t by_classify, by_correct, by_overflow;
	double ms_scan;             /* device time of the length kernel + the scan, and of the gather                   */
	double ms_gather;
} dbgk_corr_compact_info;
/* dbgk_corr_reads for reads already in device memory of the handle's GPU: d_seq (16-byte aligned, offsets[n] bytes, not
 * written) is read where it lies.  offsets are HOST memory as above; out_rec is written as above, the corrected bytes stay
 * on the device for dbgk_corr_compact.  The call returns when the batch is done.                                            */
int dbgk_corr_reads_device(dbgk_corr *c, const char *d_seq, const uint64_t *offsets, uint64_t n, dbgk_corr_rec *out_rec);
/* the compact batch of the handle's last batch (dbgk_corr_reads, dbgk_corr_reads_device, dbgk_corr_compact_from); before any:
 * DBGK_ERR_STATE.  Returns when it is complete.                                                                             */
int dbgk_corr_compact(dbgk_corr *c, dbgk_corr_compact_info *out);
/* the same for a batch the caller holds on the host -- what an earlier dbgk_corr_reads returned: untrimmed corrected bytes,
 * offsets (checked as there), records.  It becomes the handle's batch; no table is needed.                                  */
int dbgk_corr_compact_from(dbgk_corr *c, const char *seq, const uint64_t *offsets, const dbgk_corr_rec *rec, uint64_t n,
                           dbgk_corr_compact_info *out);
/* host copy of the compact batch: offsets[n] bytes (without the pad) and n + 1 offsets                                      */
int dbgk_corr_compact_results(dbgk_corr *c, char *bases, uint64_t *offsets);
/* the compact batch where it lies; valid until the next dbgk_corr_reads*, dbgk_corr_compact* or dbgk_corr_destroy on c       */
int dbgk_corr_compact_device(dbgk_corr *c, const char **d_bases, const uint64_t **d_offsets, uint64_t *n_reads, uint64_t *n_bases);
/* dbgk_push_reads_device of c's compact batch into h (any engine that call serves, KFREQ included), ordered by events: h's
 * stream waits for the compaction, and c waits for the event recorded on h's stream behind the push before it overwrites,
 * regrows or frees the compact buffers -- so c may be used again at once.  Every kernel that reads the pushed pointers is
 * queued on h's stream by the push itself (the record engines keep records, no engine keeps the pointers), so that event
 * covers them all and the call does not end with a dbgk_sync.  One compact batch may be pushed into several handles (a KFREQ
 * handle and a graph, say): each push makes h's stream wait for the event of the push before it, so the latest event lies
 * behind every reader.  Handles on different devices: DBGK_ERR_ARG; no compact batch, or h finalized: DBGK_ERR_STATE.       */
int dbgk_push_corrected(dbgk_handle *h, dbgk_corr *c);

/* The annotation of the headers, composed on the device (additions to ABI 7).  For record i of the compact batch the suffix is what
 * bin/correct_error_reads appends to header i, without the final "\n":
 *   "\tModifiedBaseNum: " M "\tFinalReadLength: " F "\tLeftEndTrim: " Lt "\tRightEndTrim: " Rt "\tIsDeleted: " D
 * M = (uint32)(one_base + tree), F = the record's length in the compact batch, Lt / Rt = left_trim / right_trim as stored, D =
 * deleted as an unsigned number, all in decimal without padding.  The plane has the layout of every other plane: from a 16-byte
 * boundary in whole 16-byte vectors, the pad of the last one 0, 64 readable bytes behind it, n + 1 64-bit offsets from 0 -- what
 * dbgk_fmt_records_device_suffix reads where it lies.  A suffix has at most DBGK_CORR_ANNOT_MAX bytes: the 77 bytes of the literals,
 * four numbers of 10 digits and one of 3.                                                                                  */
#define DBGK_CORR_ANNOT_MAX 120
typedef struct dbgk_corr_annot_info {
	uint64_t n;                 /* records                                                                              */
	uint64_t suffix_bytes;      /* bytes of the plane (without the pad)                                                 */
	double ms_scan;             /* device time of the length kernel + the scan, and of the write kernel                 */
	double ms_write;
} dbgk_corr_annot_info;
/* the plane of the handle's compact batch (dbgk_corr_compact, dbgk_corr_compact_from); before one: DBGK_ERR_STATE.  Returns when it
 * is complete.                                                                                                             */
int dbgk_corr_annot(dbgk_corr *c, dbgk_corr_annot_info *out);
/* the plane where it lies; valid until the next dbgk_corr_reads*, dbgk_corr_compact*, dbgk_corr_annot or dbgk_corr_destroy on c.
 * Before a dbgk_corr_annot of the current compact batch: DBGK_ERR_STATE (also for dbgk_corr_annot_results).                 */
int dbgk_corr_annot_device(dbgk_corr *c, const char **d_suffix, const uint64_t **d_suffix_offsets, uint64_t *n, uint64_t *n_bytes);
/* host copy: suffix_bytes bytes (without the pad) and n + 1 offsets; either pointer may be null                            */
int dbgk_corr_annot_results(dbgk_corr *c, char *suffix, uint64_t *suffix_offsets);

/* ---- MAP: map_reads / map_pair of the link_scaffold module on the GPU (additions to ABI 7) ----------------------------------
 * The reference maps every read onto the contigs with a seed search over the contig k-mer index (get_align_seed,
 * link_scaffold/map_func.cpp:181-237) and a gap-free extension with a mismatch count (extend_align_region, :241-299).  A mapper
 * owns the finalized seed index of its contigs (built through DBGK_ENGINE_SEEDIDX with find_next_prime(3 * total length) slots,
 * map_pair.cpp:122), the contig text as written (the extension compares raw bytes) and staging for read batches.  Every hit
 * equals the reference's for the same contigs, read and options; the identity test is bit-equal to its float expression.   */
typedef struct dbgk_map dbgk_map;

typedef struct dbgk_map_params {
	int32_t k;                  /* -k KmerSize, 1..31                                                               */
	int32_t seed_kmers;         /* -s SeedKmerNum, >= 1                                                             */
	int32_t min_read_len;       /* -r MinReadLen, >= 0: shorter reads get two empty hits                            */
	int32_t second_alignment;   /* 1: map_reads (the rest of a read behind an accepted alignment is mapped again,
	                               map_reads.cpp:480-498), 0: map_pair (every mate is simply a read)                */
	double  min_identity;       /* -i MinMapIdentity                                                                */
} dbgk_map_params;

/* coordinates 1-based inclusive, as the reference prints them.  No seed: contig -1, coordinates -1, direct 'N', align_len 0.
 * Seed found but identity below min_identity: contig -1, everything else as computed.                                   */
typedef struct dbgk_map_hit {
	int32_t contig;
	int32_t read_start, read_end, contig_start, contig_end;
	int32_t mismatches, align_len;  /* identity = 1.0 - (float)mismatches / align_len (map_func.cpp:298)             */
	int32_t direct;                 /* 'F' / 'R' / 'N'                                                               */
} dbgk_map_hit;

typedef struct dbgk_map_stats {
	uint64_t reads;
	uint64_t by_lds;            /* reads mapped out of LDS (up to 1024 bases)                                       */
	uint64_t by_long;           /* longer reads, mapped out of global memory                                        */
	uint64_t skipped;           /* reads shorter than min_read_len or than k + seed_kmers                           */
	uint64_t windows_probed;    /* first k-mers of a seed looked up in the index, speculative ones included         */
	double ms_map, ms_long;     /* device time of each kernel of the last batch                                     */
} dbgk_map_stats;

/* DBGK_ERR_ARG on a bad parameter, before any device work */
int dbgk_map_create(const dbgk_map_params *p, int device, dbgk_map **out);
int dbgk_map_destroy(dbgk_map *m);
/* n_contigs sequences back to back, contig i = bases[offsets[i], offsets[i+1]) (offsets[0] == 0, each < 2^30 bytes; empty ones
 * keep their index and match nothing).  Replaces the mapper's earlier contigs.                                            */
int dbgk_map_set_contigs(dbgk_map *m, const char *bases, const uint64_t *offsets, uint64_t n_contigs);
/* the seed scan looks at first_chunk (1..64) windows of a read at once, then at 64 at a time (default 4)                  */
int dbgk_map_set_ramp(dbgk_map *m, uint32_t first_chunk);
/* n_reads reads laid out like the contigs (each < 2^31 bytes); out: 2 hits per read, the second one only ever set with
 * second_alignment.  Input order is kept.                                                                                 */
int dbgk_map_reads(dbgk_map *m, const char *bases, const uint64_t *offsets, uint64_t n_reads, dbgk_map_hit *out);
int dbgk_map_batch_stats(dbgk_map *m, dbgk_map_stats *out);
/* dbgk_map_reads for a batch in device memory of the mapper's GPU, offsets included -- a PAIR output (dbgk_pair_device), or a
 * compact batch of the corrector or the cleaner: read 2i and 2i + 1 of a PAIRED output are pair i.  d_bases (16-byte aligned)
 * holds n_bases bytes and must be readable for 16 bytes behind them, as the PAIR and compact planes are for 64; d_offsets are
 * n_reads + 1 offsets into it, non-decreasing, the last one <= n_bases.  max_len >= the longest read sizes the identity table
 * (dbgk_pair_info.max_len; any upper bound will do).  The offsets are checked on the device before a read is mapped: a read
 * longer than max_len, offsets that decrease or an end behind n_bases give DBGK_ERR_ARG and no hits.  Work of the caller's own on
 * the batch has to be synchronised; the call returns when the hits are in `out`.                                           */
int dbgk_map_reads_device(dbgk_map *m, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t max_len,
                          dbgk_map_hit *out);
/* dbgk_map_reads_device without the copy to the host: the hits stay in the mapper's buffer for dbgk_map_hits_device and
 * dbgk_maprow_take_hits.  Same checks, same statistics.                                                                    */
int dbgk_map_reads_device_keep(dbgk_map *m, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t max_len);
/* the 2 n_reads hits of the last batch (any of the three calls) where they lie; valid until the next batch, dbgk_map_set_contigs or
 * dbgk_map_destroy.  Before a successful batch: DBGK_ERR_STATE.  *d_hits is null when n_reads is 0.                          */
int dbgk_map_hits_device(dbgk_map *m, const dbgk_map_hit **d_hits, uint64_t *n_reads);

/* ---- CLEAN: clean_adapter / clean_lowqual of the clean_illumina module on the GPU (additions to ABI 7) -------------------------
 * clean_adapter aligns every read against every contaminant sequence with an ungapped local dynamic programme (match +1,
 * everything else -2, N against N included; local_ungapped_aligning, clean_illumina/clean_adapter.cpp:94-157) and cuts the read at
 * the first contaminant whose best score reaches the cutoff (:189-206).  clean_lowqual sums the per-base error probabilities of a
 * read and, when their mean exceeds the cutoff, keeps the first longest block between break points (clean_lowqual.cpp:84-160).
 * The device returns the numbers; headers, cutting, the short-read filter, statistics and gzip are the caller's (bin/clean_adapter,
 * bin/clean_lowqual, capi.Cleaner).  Every number equals the reference's for the same input and options, doubles bit for bit.  */
typedef struct dbgk_clean dbgk_clean;

/* 1-based, inclusive, exactly the numbers the reference prints.  No contaminant reaches the cutoff: adapter -1, the rest 0.     */
typedef struct dbgk_adapter_hit {
	int32_t adapter;            /* index of the FIRST contaminant whose best score reaches the cutoff (not the best of all)    */
	int32_t score;              /* score of the first cell in row-major order that holds that contaminant's maximum            */
	int32_t read_start, read_end, adapter_start, adapter_end;
} dbgk_adapter_hit;

typedef struct dbgk_lowqual_block {
	double  error_sum;          /* sum of the per-base error probabilities over the whole read, added left to right            */
	int32_t start, length;      /* 1-based start and length of what is kept: the first longest block when trimmed (start 0:
	                               nothing kept), else the whole read (start 1, or 0 for an empty read)                        */
	int32_t trimmed;            /* 1 when error_sum > cutoff * read_len                                                        */
	int32_t reserved;
} dbgk_lowqual_block;

typedef struct dbgk_clean_stats {  /* of the last dbgk_clean_adapter / dbgk_clean_lowqual call                                  */
	uint64_t reads;
	uint64_t by_lds;            /* reads aligned out of LDS (up to 1024 bases, contaminant set of up to 4096 bases)            */
	uint64_t by_global;         /* longer reads, or every read of a larger contaminant set: the same code out of global memory */
	uint64_t hits;              /* reads with a contaminant at or above the cutoff                                             */
	uint64_t cells;             /* read_len * contaminant_len summed over every pair that was aligned                          */
	double ms_lds, ms_global;   /* device time of each form of the adapter kernel                                              */
	double ms_lowqual;          /* device time of the low-quality kernel                                                       */
} dbgk_clean_stats;

/* DBGK_ERR_HIP without a usable gfx950 device: there is no host fall-back                                                      */
int dbgk_clean_create(int device, dbgk_clean **out);
int dbgk_clean_destroy(dbgk_clean *c);
/* n contaminant sequences in the order they are tried, back to back, sequence i = bases[offsets[i], offsets[i+1]) (offsets[0] == 0);
 * score_cutoff >= 1 (-s; below 1 the reference reports coordinates it never set).  Replaces the earlier set.                    */
int dbgk_clean_set_adapters(dbgk_clean *c, const char *bases, const uint64_t *offsets, uint64_t n, int32_t score_cutoff);
/* n_reads reads laid out the same way (each < 2^30 bytes); out: one hit per read, input order kept                              */
int dbgk_clean_adapter(dbgk_clean *c, const char *bases, const uint64_t *offsets, uint64_t n_reads, dbgk_adapter_hit *out);
/* bases and quals share the offsets (a record whose two strings differ in length is the caller's to empty first);
 * quality_shift 0..127 (-q), error_rate_cutoff -e; out: one block per read                                                      */
int dbgk_clean_lowqual(dbgk_clean *c, const char *bases, const char *quals, const uint64_t *offsets, uint64_t n_reads,
                       double error_rate_cutoff, int32_t quality_shift, dbgk_lowqual_block *out);
int dbgk_clean_batch_stats(dbgk_clean *c, dbgk_clean_stats *out);

/* The cleaned reads stay on the device (additions to ABI 7).  The COMPACT batch is what the two programs write as lines 2 and 4
 * of every record, without the text.  After a lowqual batch the quality of every byte 'N' of a read becomes (char)quality_shift,
 * and a read with `trimmed` is its bytes [start - 1, start - 1 + length), or nothing when start == 0; after an adapter batch a
 * read with adapter >= 0 is its first read_start - 1 bytes and no quality is rewritten.  In both a result shorter than min_len
 * becomes empty, and a record that points outside its read (the kernels write none) gives length 0: no byte outside a read is
 * ever copied.  The reads lie back to back in input order, an emptied read of length 0 at its place (pairs stay pairs); bases
 * and qualities are two planes under one set of n + 1 64-bit offsets.  Each plane starts on a 16-byte boundary and fills whole
 * 16-byte vectors, the pad of the last one 0: the layout of dbgk_corr_compact.  The gather kernel works in tiles of
 * DBGK_CLEAN_COMPACT_TILE output bytes of each plane.                                                                        */
#define DBGK_CLEAN_COMPACT_TILE 4096
#define DBGK_CLEAN_KIND_LOWQUAL 0   /* the records are dbgk_lowqual_block                                                     */
#define DBGK_CLEAN_KIND_ADAPTER 1   /* the records are dbgk_adapter_hit                                                       */
typedef struct dbgk_clean_compact_info {
	/* the integer columns of the .stat file of the program the batch came from (one batch = one file).  With m the length of a
	 * read's result before the short-read filter: trimmed_bases adds L - m per trimmed read, which on the kernels' records is
	 * clean_adapter's read_len - read_start + 1 per hit and clean_lowqual's seq_len - length per trimmed read; clean_reads counts
	 * every read that is not short after an adapter batch (empty ones included when min_len is 0), only non-empty reads after a
	 * lowqual batch.                                                                                                           */
	uint64_t reads, raw_bases;
	uint64_t trimmed_reads, trimmed_bases;
	uint64_t short_reads, short_bases;
	uint64_t clean_reads, clean_bases;
	double ms_scan;             /* device time of the length kernel + the scan, and of the gather                            */
	double ms_gather;
} dbgk_clean_compact_info;
/* dbgk_clean_lowqual / dbgk_clean_adapter for a batch already in device memory of the handle's GPU: d_bases and d_quals (16-byte
 * aligned, never written) are read where they lie and must be readable for 16 bytes behind offsets[n], as the handle's own
 * batch buffers are (the kernels load whole dwords); they must stay valid until the batch has been compacted.  offsets are HOST
 * memory; out gets the n records as above.  d_quals of the adapter call may be null: the compact batch then has no quality
 * plane.  Passing the handle's own compact planes is DBGK_ERR_ARG: a chain of two stages uses two handles.  The calls return
 * when the batch is done.                                                                                                    */
int dbgk_clean_lowqual_device(dbgk_clean *c, const char *d_bases, const char *d_quals, const uint64_t *offsets, uint64_t n_reads,
                              double error_rate_cutoff, int32_t quality_shift, dbgk_lowqual_block *out);
int dbgk_clean_adapter_device(dbgk_clean *c, const char *d_bases, const char *d_quals, const uint64_t *offsets, uint64_t n_reads,
                              dbgk_adapter_hit *out);
/* the compact batch of the handle's last batch (any of the four calls above, or dbgk_clean_compact_from); before any:
 * DBGK_ERR_STATE.  min_len >= 0 is the programs' -r.  Returns when it is complete.                                           */
int dbgk_clean_compact(dbgk_clean *c, int32_t min_len, dbgk_clean_compact_info *out);
/* the same for a batch the caller holds on the host: reads, qualities (may be null: no quality plane) and the records of an
 * earlier call, `kind` naming their type; quality_shift is used by DBGK_CLEAN_KIND_LOWQUAL only.  It becomes the handle's batch. */
int dbgk_clean_compact_from(dbgk_clean *c, int32_t kind, const char *bases, const char *quals, const uint64_t *offsets, const void *recs,
                            uint64_t n_reads, int32_t quality_shift, int32_t min_len, dbgk_clean_compact_info *out);
/* host copy of the compact batch: offsets[n] bytes of each plane (without the pad) and n + 1 offsets.  Any of the three may be
 * null; quals of a batch without a quality plane: DBGK_ERR_ARG.                                                              */
int dbgk_clean_compact_results(dbgk_clean *c, char *bases, char *quals, uint64_t *offsets);
/* the compact batch where it lies (*d_quals null without a quality plane); valid until the handle's next batch, next compact
 * or dbgk_clean_destroy                                                                                                      */
int dbgk_clean_compact_device(dbgk_clean *c, const char **d_bases, const char **d_quals, const uint64_t **d_offsets, uint64_t *n_reads,
                              uint64_t *n_bases);
/* dbgk_push_reads_device of c's compact bases into h (any engine that call serves, KFREQ included), ordered by events as
 * dbgk_push_corrected is: h's stream waits for the compaction, and c waits for the event recorded on h's stream behind the push
 * before it overwrites, regrows or frees the compact buffers -- so c may be used again at once.  One compact batch may be pushed
 * into several handles: each push makes h's stream wait for the event of the push before it, so the latest event lies behind
 * every reader.  Handles on different devices: DBGK_ERR_ARG; no compact batch, or h finalized: DBGK_ERR_STATE.                */
int dbgk_push_cleaned(dbgk_handle *h, dbgk_clean *c);

/* ---- PAIR: read pairs through the device pipeline (additions to ABI 7) -----------------------------------------------------------
 * The compact batches of the corrector and the cleaner keep an emptied read at its place with length 0, so that mate 1 and mate 2 of
 * pair i stay at index i of their two batches.  The PAIR stage splits two such batches of n reads each the way
 * merge_two_corr_files does (correct_error/correct.cpp:851-922; clean_illumina/filter_unpaired_reads.pl states the same rule):
 *   PAIRED  for every i with both mates not empty: mate 1, then mate 2, in index order;
 *   SINGLE  for every other i: mate 1 if it is not empty, then mate 2 if it is not empty, in index order.
 * Both outputs have the layout of dbgk_corr_compact / dbgk_clean_compact -- each plane from a 16-byte boundary in whole 16-byte
 * vectors, the pad of the last one 0, 64 readable bytes behind the end, n_reads + 1 64-bit offsets -- so dbgk_push_reads_device and
 * dbgk_map_reads_device read them where they lie.  Per output read there is a source id 2 i + mate (mate 0 or 1), by which a
 * caller attaches headers.  Both inputs have a quality plane or neither has; the outputs then have one or none.            */
typedef struct dbgk_pair dbgk_pair;
#define DBGK_PAIR_PAIRED 0
#define DBGK_PAIR_SINGLE 1
typedef struct dbgk_pair_info {
	uint64_t n_pairs_in;        /* n                                                                                    */
	uint64_t pair_reads;        /* the four numbers of <file>.pair.single.stat: reads (2 per kept pair) and bases of    */
	uint64_t pair_bases;        /* PAIRED, reads and bases of SINGLE                                                    */
	uint64_t single_reads;
	uint64_t single_bases;
	uint64_t max_len;           /* the longest read of both outputs (0: both are empty): dbgk_map_reads_device's max_len */
	double ms_rank;             /* device time of classify + scans + scatter + offset scans, and of both gathers        */
	double ms_gather;
} dbgk_pair_info;
/* DBGK_ERR_HIP without a usable gfx950 device: there is no host fall-back                                                  */
int dbgk_pair_create(int device, dbgk_pair **out);
int dbgk_pair_destroy(dbgk_pair *p);
/* two batches on the host, uploaded by the call: read i of mate file m = bases<m>[offsets<m>[i], offsets<m>[i + 1]) (offsets<m>[0]
 * == 0, non-decreasing, each read < 2^31 bytes, n < 2^31); quals1 and quals2 are both null or both set and share the offsets of
 * their bases.  n == 0 and inputs or outputs without a read are valid.  Returns when both outputs are complete.            */
int dbgk_pair_split_from(dbgk_pair *p, const char *bases1, const char *quals1, const uint64_t *offsets1, const char *bases2,
                         const char *quals2, const uint64_t *offsets2, uint64_t n, dbgk_pair_info *out);
/* the same for batches in device memory of p's GPU, offsets included -- what dbgk_corr_compact_device / dbgk_clean_compact_device
 * of two handles return (those calls return synchronised; work of the caller's own on the inputs has to be synchronised too).
 * The planes must be 16-byte aligned (else DBGK_ERR_ARG), are never written, and are read only inside the whole dwords of
 * [offsets[0] & ~3, offsets[n]); offsets[0] need not be 0.  The stage's own output planes as input: DBGK_ERR_ARG.  Offsets that
 * decrease or a read of 2^31 bytes and more are found on the device: DBGK_ERR_ARG, no output.                                */
int dbgk_pair_split_device(dbgk_pair *p, const char *d_bases1, const char *d_quals1, const uint64_t *d_offsets1, const char *d_bases2,
                           const char *d_quals2, const uint64_t *d_offsets2, uint64_t n, dbgk_pair_info *out);
/* host copy of one output (which: DBGK_PAIR_PAIRED / DBGK_PAIR_SINGLE): offsets[n_reads] bytes of each plane (without the pad),
 * n_reads + 1 offsets, n_reads source ids.  Any pointer may be null; quals of an output without a quality plane: DBGK_ERR_ARG.
 * Before a successful split: DBGK_ERR_STATE (also for the two calls below).                                                */
int dbgk_pair_results(dbgk_pair *p, int which, char *bases, char *quals, uint64_t *offsets, uint32_t *src_ids);
/* one output where it lies (*d_quals null without a quality plane); valid until the next split or dbgk_pair_destroy        */
int dbgk_pair_device(dbgk_pair *p, int which, const char **d_bases, const char **d_quals, const uint64_t **d_offsets, uint64_t *n_reads,
                     uint64_t *n_bases);
/* dbgk_push_reads_device of one output into h (any engine that call serves), ordered by events as dbgk_push_corrected is: p may
 * start its next split at once, and one output may be pushed into several handles.  Handles on different devices: DBGK_ERR_ARG;
 * no split yet, or h finalized: DBGK_ERR_STATE.                                                                           */
int dbgk_push_pairs(dbgk_handle *h, dbgk_pair *p, int which);

/* ---- PARSE: from a FASTQ / FASTA file's bytes to the device batch (additions to ABI 7) ---------------------------------------------
 * The stage in front of the first stage: the caller uploads the text of the file as it is (a gz file through dbgk_inf_inflate first), the handle
 * finds the records on the device and leaves the batch in the layout of dbgk_corr_compact / dbgk_clean_compact -- each plane from a
 * 16-byte boundary in whole 16-byte vectors, the pad of the last one 0, 64 readable bytes behind the end, n + 1 64-bit offsets -- so
 * dbgk_clean_*_device, dbgk_corr_reads_device, dbgk_pair_split_device, dbgk_push_reads_device and dbgk_map_reads_device read it where it
 * lies.  The record rule is the one of both host readers (DBG_contig/DBGgraph.cpp:244-272, clean_illumina/clean_adapter.cpp:376-387):
 *   - a line ends at '\n'; a '\r' in front of it belongs to the line; the last line of the input may lack its '\n';
 *   - state 0 looks for a header: a line that is not empty and begins with the marker ('@' for format 1, '>' for format 2) opens a
 *     record, any other line is ignored; the next line is the sequence; FASTQ then passes a separator and a quality line whatever
 *     they begin with; single-line FASTA only, as in the reference;
 *   - a record exists once its header has been seen: lines the input lacks at its end are empty;
 *   - with a quality plane (FASTQ only) a record whose sequence and quality lines differ in length is emptied in both planes and
 *     counted, as bin/clean_lowqual does; without one the quality line is not looked at.
 * A chunk is parsed on its own, from state 0.  With last == 0 only records whose lines all end with a newline inside the chunk are
 * delivered, and `consumed` is the first byte not used up -- the header of the first incomplete record, or, if the chunk ends in
 * state 0, the byte behind its last newline; the caller presents the bytes from there on again at the front of its next chunk.
 * consumed == 0 with no record is a valid answer: the chunk is smaller than one record.  With last != 0 the final line needs no
 * newline, an incomplete record is delivered with its missing lines empty, and consumed == n_bytes.  The counters of the chunks of a
 * stream add up to those of the whole text.                                                                                */
typedef struct dbgk_parse dbgk_parse;
#define DBGK_PARSE_TEXT_TILE 4096   /* bytes of text per workgroup round of the line kernels                              */
typedef struct dbgk_parse_rec {     /* the lines of one record, relative to the chunk; a missing line: n_bytes, 0; FASTA: no */
	uint32_t head_pos, head_len, seq_pos, seq_len, qual_pos, qual_len; /* quality line (0, 0).  As the text has them, also   */
} dbgk_parse_rec;                   /* for a record that was emptied                                                      */
typedef struct dbgk_parse_info {
	uint64_t n_records;         /* records delivered                                                                    */
	uint64_t n_lines;           /* lines in front of `consumed`                                                         */
	uint64_t ignored_lines;     /* ... of which met in state 0 without being a header                                   */
	uint64_t consumed;
	uint64_t n_bases;           /* bytes of each plane                                                                  */
	uint64_t max_len;           /* the longest read delivered: dbgk_map_reads_device's max_len                          */
	uint64_t mismatched;        /* records emptied because sequence and quality differ in length                        */
	double ms_lines;            /* device time: newline count + scan + line table; map scan + flags + rank;             */
	double ms_states;           /* records + offsets; the gathers                                                       */
	double ms_scan;
	double ms_gather;
} dbgk_parse_info;
/* format 1 FASTQ, 2 FASTA; with_quals: the batch has a quality plane (format 1 only, else DBGK_ERR_ARG).  DBGK_ERR_HIP without a
 * usable gfx950 device: there is no host fall-back                                                                         */
int dbgk_parse_create(int32_t format, int32_t with_quals, int device, dbgk_parse **out);
int dbgk_parse_destroy(dbgk_parse *p);
/* one chunk of text on the host, uploaded by the call.  n_bytes < 2^31 (else DBGK_ERR_ARG); n_bytes == 0 is valid.  Returns when
 * the batch is complete.                                                                                                   */
int dbgk_parse_chunk(dbgk_parse *p, const char *text, uint64_t n_bytes, int32_t last, dbgk_parse_info *out);
/* the same for text in device memory of p's GPU, read in place and never written: d_text 16-byte aligned (else DBGK_ERR_ARG) and
 * readable up to n_bytes rounded up to 16; no byte at or behind n_bytes influences a result.  The handle's own planes as input:
 * DBGK_ERR_ARG.  Work of the caller's own on the text has to be synchronised.                                              */
int dbgk_parse_chunk_device(dbgk_parse *p, const char *d_text, uint64_t n_bytes, int32_t last, dbgk_parse_info *out);
/* host copy of the batch: n_bases bytes of each plane (without the pad), n_records + 1 offsets -- the host copy that
 * dbgk_clean_lowqual_device and dbgk_corr_reads_device ask for --, n_records records.  Any pointer may be null; quals of a batch
 * without a quality plane: DBGK_ERR_ARG.  Before a successful chunk: DBGK_ERR_STATE (also for the two calls below).        */
int dbgk_parse_results(dbgk_parse *p, char *bases, char *quals, uint64_t *offsets, dbgk_parse_rec *recs);
/* the batch where it lies (*d_quals null without a quality plane); valid until the next chunk or dbgk_parse_destroy        */
int dbgk_parse_device(dbgk_parse *p, const char **d_bases, const char **d_quals, const uint64_t **d_offsets, uint64_t *n_reads,
                      uint64_t *n_bases);
/* dbgk_push_reads_device of the batch into h, ordered by events as dbgk_push_corrected is: p may start its next chunk at once.
 * Handles on different devices: DBGK_ERR_ARG; no batch, or h finalized: DBGK_ERR_STATE.                                    */
int dbgk_push_parsed(dbgk_handle *h, dbgk_parse *p);

/* ---- GZ: deflate on the GPU, the output as BGZF-framed gzip members (additions to ABI 7) -------------------------------------------
 * The text of a call is cut into pieces of at most 65 280 bytes, every piece but the last exactly that long, and every piece becomes
 * one gzip member of its own: the 18-byte header 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, the subfield 42 43 02 00 and BSIZE
 * (u16, the member's size - 1); ONE deflate block with BFINAL set; CRC-32 and ISIZE of the piece.  Concatenated members are a
 * valid gzip file (zlib's gzread, Python's gzip and bgzip read them), and BSIZE makes the file self-delimiting.  With last != 0 the
 * 28-byte BGZF end marker follows the members; empty input gives the marker alone, or nothing with last == 0.  Calls are stateless:
 * no history, code or checksum carries over, and a short last member per call is fine.  Levels, fixed at creation:
 *   0  stored blocks;
 *   1  one dynamic-Huffman block of literals only;
 *   2  dynamic Huffman over LZ77 tokens (the default of the Python binding and the bin/ programs): matches of length 3..258 at
 *      distance 1..32 768 that never reach into another member or past the piece's end, chosen by a deterministic rule.
 * At levels 1 and 2 a member whose dynamic block would not be smaller than its stored block is written stored.  Fixed-Huffman blocks
 * are not used.  The same input gives the same bytes on every run.
 * The members are independent, which is what lets them be built (and inflated: the INFLATE section) in parallel and costs the size DESIGN.md
 * states.  The construction rules of the codes are DESIGN.md's; CRC-32 is computed on the device.                              */
typedef struct dbgk_gz dbgk_gz;
typedef dbgk_gz *dbgk_gz_t;
#define DBGK_GZ_PIECE 65280         /* bytes of text per member                                                             */
#define DBGK_GZ_MAX_LEVEL 2
typedef struct dbgk_gz_info {
	uint64_t n_members;         /* members with text: ceil(n_bytes / 65280); the end marker is not counted              */
	uint64_t out_bytes;         /* all bytes of the call's output, the marker included                                  */
	uint64_t stored_members;    /* members written with a stored block                                                  */
	uint64_t n_literals;        /* literal tokens of the dynamic blocks (a stored member has no tokens)                 */
	uint64_t n_matches;         /* match tokens of the dynamic blocks and the bytes they cover (0 at levels 0 and 1)    */
	uint64_t match_bytes;
} dbgk_gz_info;
typedef struct dbgk_gz_timing {     /* device time of the last call.  A member is built by ONE launch from the piece in LDS, */
	double ms_members;          /* timed by events; its phases are that time divided by the shares of the shader-clock   */
	double ms_match;            /* cycles that lane 0 of every workgroup counted between them: the matcher (level 2;     */
	double ms_crc_hist;         /* else 0); staging,      CRC-32 and the histogram, which are one pass over the piece;   */
	double ms_codes;            /* ranking, code lengths, codes and the block header; bit count, scan, zeroing and       */
	double ms_encode;           /* encoding.  ms_match + ms_crc_hist + ms_codes + ms_encode == ms_members.               */
	double ms_compact;          /* the scan of the sizes and the gather, by events                                       */
} dbgk_gz_timing;
/* on the current device.  A level outside 0..DBGK_GZ_MAX_LEVEL: DBGK_ERR_ARG, before any device work.  DBGK_ERR_HIP without a
 * usable gfx950 device: there is no host fall-back                                                                         */
int dbgk_gz_create(int level, dbgk_gz_t *out);
int dbgk_gz_destroy(dbgk_gz_t z);
/* text on the host, uploaded by the call.  n_bytes < 2^31 (else DBGK_ERR_ARG); n_bytes == 0 is valid.  info may be null.  Returns
 * when the output is complete.                                                                                             */
int dbgk_gz_deflate(dbgk_gz_t z, const void *text, uint64_t n_bytes, int last, dbgk_gz_info *info);
/* the same for text in device memory of z's GPU, read in place and never written: d_text 16-byte aligned (else DBGK_ERR_ARG) and
 * readable up to n_bytes rounded up to 16; no byte at or behind n_bytes influences a result.  The handle's own output as input:
 * DBGK_ERR_ARG.  Work of the caller's own on the text has to be synchronised.                                              */
int dbgk_gz_deflate_device(dbgk_gz_t z, const void *d_text, uint64_t n_bytes, int last, dbgk_gz_info *info);
/* host copy of the output of the last call: out_bytes bytes; a capacity below that: DBGK_ERR_ARG.  Before a successful call:
 * DBGK_ERR_STATE (also for dbgk_gz_device).                                                                                */
int dbgk_gz_results(dbgk_gz_t z, void *out, uint64_t capacity);
/* the output where it lies (null if it is empty); valid until the next call or dbgk_gz_destroy                             */
int dbgk_gz_device(dbgk_gz_t z, const void **d_out, uint64_t *n_out);
int dbgk_gz_timing_get(dbgk_gz_t z, dbgk_gz_timing *t);

/* ---- INFLATE: inflate on the GPU, BGZF-framed gzip members decoded in parallel (additions to ABI 7) --------------------------------
 * The reader that the GZ section's members were made independent for.  Input: gzip members in exactly that section's framing -- the
 * 16 fixed header bytes, BSIZE, a deflate stream, CRC-32 and ISIZE <= 65 280 -- back to back; htslib's bgzip writes the same 16
 * bytes, so its files are accepted too.  The stream inside a member may be anything RFC 1951 allows: stored, fixed and dynamic
 * blocks, any number of them, empty stored blocks of a flush, codes of up to 15 bits, a distance code of one symbol or none,
 * matches that overlap themselves, distances of up to 32 768.  Output: the members' bytes back to back, on the device.
 * Every member gets a verdict: 0, or the first reason below for which it was refused.  What zlib accepts is accepted, what it refuses
 * is refused.  A refused member's range of the output is zero bytes and no other member is disturbed; a call that ran returns
 * DBGK_OK whatever the verdicts, n_bad counts them.  The same input gives the same bytes, verdicts and counters on every run.
 * Temporary device memory is the token area: 4 000 members x 65 280 tokens x 4 bytes = 1 044 480 000 bytes at the most, whatever the
 * size of the call; members are processed in rounds of 4 000.  (28 bytes of table and verdict per member come on top.)
 * Calls are stateless apart from buffers.  There is no host fall-back inside the library.                                        */
typedef struct dbgk_inf dbgk_inf;
typedef dbgk_inf *dbgk_inf_t;
#define DBGK_INF_ROUND 4000             /* members per round of the token area                                                */
#define DBGK_INF_OK 0
#define DBGK_INF_BLOCK_TYPE 1           /* block type 3                                                                       */
#define DBGK_INF_STORED_LEN 2           /* a stored block's LEN is not the complement of its NLEN                             */
#define DBGK_INF_STORED_PAST 3          /* a stored block's LEN runs past the member                                          */
#define DBGK_INF_TOO_MANY_SYMS 4        /* HLIT above 286 or HDIST above 30                                                   */
#define DBGK_INF_CL_OVER 5              /* the code of the code lengths is over-subscribed                                    */
#define DBGK_INF_CL_INCOMPLETE 6        /* ... or incomplete                                                                  */
#define DBGK_INF_CODE_OVER 7            /* the literal/length or the distance code is over-subscribed                         */
#define DBGK_INF_CODE_INCOMPLETE 8      /* ... or incomplete and not a single code of one bit                                 */
#define DBGK_INF_REPEAT_FIRST 9         /* repeat code 16 as the first length                                                 */
#define DBGK_INF_REPEAT_PAST 10         /* a repeat that runs past HLIT + HDIST                                               */
#define DBGK_INF_NO_EOB 11              /* no code for symbol 256                                                             */
#define DBGK_INF_BAD_LENGTH 12          /* length symbol 286 or 287, or bits that are no literal/length code                  */
#define DBGK_INF_BAD_DISTANCE 13        /* distance symbol 30 or 31, or bits that are no distance code                        */
#define DBGK_INF_DISTANCE_FAR 14        /* a distance that reaches in front of the member's first byte                        */
#define DBGK_INF_TRUNCATED 15           /* the stream ends in mid-symbol at the trailer                                       */
#define DBGK_INF_GARBAGE 16             /* the final block ends before the trailer                                            */
#define DBGK_INF_OUT_MORE 17            /* more output than ISIZE                                                             */
#define DBGK_INF_OUT_LESS 18            /* less output than ISIZE                                                             */
#define DBGK_INF_CRC 19                 /* the CRC-32 of the output is not the trailer's                                      */
#define DBGK_INF_FRAME 20               /* dbgk_inf_inflate_device: no member of this framing where the table says one is     */
typedef struct dbgk_inf_info {
	uint64_t n_members;         /* members inflated by the call (end markers and other ISIZE-0 members included)        */
	uint64_t n_markers;         /* ... of which the 28-byte end marker, byte for byte                                   */
	uint64_t consumed;          /* bytes of input used up: whole members only                                           */
	uint64_t out_bytes;
	uint64_t n_stored, n_fixed, n_dynamic;   /* blocks of the members whose streams decoded: verdict 0 or DBGK_INF_CRC    */
	uint64_t n_literals, n_matches;          /* their tokens; a byte of a stored block is a literal                     */
	uint64_t n_bad;             /* members with a verdict other than 0                                                  */
	uint64_t first_bad;         /* index of the first, and its reason                                                   */
	uint32_t first_bad_reason;
} dbgk_inf_info;
typedef struct dbgk_inf_timing {    /* device time of the last call, by events                                             */
	double ms_decode;           /* k_inf_decode, all rounds                                                             */
	double ms_resolve;          /* k_inf_resolve, all rounds                                                            */
	double ms_scan;             /* the frame check and the scan of ISIZE                                                */
} dbgk_inf_timing;
/* on the current device.  max_out_bytes: the most a call delivers; 0: the default, 2^31 - 65536, so that a result always fits one
 * chunk of the parser; above that: DBGK_ERR_ARG.  DBGK_ERR_HIP without a usable gfx950 device: there is no host fall-back      */
int dbgk_inf_create(uint64_t max_out_bytes, dbgk_inf_t *out);
int dbgk_inf_destroy(dbgk_inf_t z);
/* members on the host.  The host follows BSIZE from member to member (two bytes each), takes whole members from the front while the
 * sum of ISIZE stays within max_out_bytes, uploads them and inflates them.  info->consumed is the first byte not used up: with
 * last == 0 a member that is cut short at the end is not consumed, and the caller presents the bytes from there on again at the front
 * of its next call; with last != 0 a cut-short tail is DBGK_ERR_ARG.  Bytes that are not this framing -- plain gzip, plain text,
 * other extra subfields, ISIZE above 65 280 -- give DBGK_ERR_ARG before any device work, and dbgk_last_error() says which: that is
 * how a caller learns that the file is zlib's to read.  n_bytes < 2^31 (else DBGK_ERR_ARG); n_bytes == 0 is valid.  info may be
 * null.  Returns when the output is complete.                                                                               */
int dbgk_inf_inflate(dbgk_inf_t z, const void *gz, uint64_t n_bytes, int last, dbgk_inf_info *info);
/* the same for members in device memory of z's GPU, read in place and never written: d_gz 16-byte aligned (else DBGK_ERR_ARG);
 * member_offsets, on the host, says where each of the n_members members starts and, in its last entry, where the last one ends:
 * n_members + 1 offsets that do not decrease, the last one at most n_bytes (else DBGK_ERR_ARG).  No byte outside the members' ranges
 * is read.  A range that does not hold a member of the framing gets the verdict DBGK_INF_FRAME and no output.  A sum of ISIZE
 * above max_out_bytes, or the handle's own output as input: DBGK_ERR_ARG.  consumed is the last offset.  The members must be
 * complete in d_gz before the call: the handle works on a stream of its own that waits for no work of the caller's, so work of the
 * caller's own that writes them has to be synchronised first.                                                                */
int dbgk_inf_inflate_device(dbgk_inf_t z, const void *d_gz, uint64_t n_bytes, const uint64_t *member_offsets, uint64_t n_members,
                            dbgk_inf_info *info);
/* host copy of the output of the last call: out_bytes bytes; a capacity below that: DBGK_ERR_ARG.  Before a successful call:
 * DBGK_ERR_STATE (also for dbgk_inf_device and dbgk_inf_member_status).                                                      */
int dbgk_inf_results(dbgk_inf_t z, void *out, uint64_t capacity);
/* the output where it lies (null if it is empty): 16-byte aligned and readable up to n_bytes rounded up to 16, which is what
 * dbgk_parse_chunk_device and dbgk_gz_deflate_device ask for; valid until the next call or dbgk_inf_destroy                  */
int dbgk_inf_device(dbgk_inf_t z, const void **d_text, uint64_t *n_bytes);
/* one verdict per member of the last call; a capacity below n_members: DBGK_ERR_ARG                                          */
int dbgk_inf_member_status(dbgk_inf_t z, uint8_t *reason, uint64_t capacity);
int dbgk_inf_timing_get(dbgk_inf_t z, dbgk_inf_timing *t);

/* ---- FORMAT: from the device batch to the bytes of a FASTQ / FASTA output file (additions to ABI 7) ------------------------------------
 * The stage behind the last stage, PARSE read backwards.  Inputs, all of one batch of n records:
 *   - the source text of n_text bytes, the chunk the parser parsed, and record i's dbgk_parse_rec, of which only head_pos and head_len
 *     are used: the header line lies in the text as it stands;
 *   - a compact batch in the layout of dbgk_clean_compact / dbgk_corr_compact / dbgk_parse_device / dbgk_pair_device: a bases plane, a
 *     quality plane (format 1 only), n + 1 64-bit offsets;
 *   - an optional suffix plane ON THE HOST, uploaded by the call: bytes and n + 1 offsets that start at 0 and do not decrease, below
 *     2^32, or null for all empty.  It is what a program appends to the header, composed by the caller.
 *     dbgk_fmt_records_device_suffix takes the same plane in device memory (dbgk_corr_annot composes one there).
 * Output, record after record in input order, with H the header's bytes (a '\r' included), S the suffix, B / Q the record's bytes
 * of the two planes and L their length:
 *   format 1 (FASTQ)  H S "\n" B "\n+\n" Q "\n"        head_len + suf_len + 2 L + 5 bytes
 *   format 2 (FASTA)  H S "\n" B "\n"                  head_len + suf_len + L + 2 bytes
 * If marker != 0 and head_len > 0 the first byte of H is replaced by marker (correct_error_reads turns '@' into '>').  An emptied
 * record (L == 0) is written with its empty lines; no record is dropped.  The text starts on a 16-byte boundary, is written in whole
 * 16-byte vectors with the pad of the last one 0, and 64 readable bytes follow it, so dbgk_gz_deflate_device and
 * dbgk_parse_chunk_device read it where it lies.  n < 2^31, n_text < 2^31, every record below 2^32 bytes of output; plane offsets and
 * out_bytes are 64-bit.                                                                                                      */
typedef struct dbgk_fmt dbgk_fmt;
#define DBGK_FMT_TILE 4096          /* bytes of output per workgroup round of the gather                                  */
typedef struct dbgk_fmt_info {
	uint64_t n_records;         /* n                                                                                    */
	uint64_t out_bytes;         /* bytes of the text (without the pad)                                                  */
	uint64_t head_bytes;        /* ... of which header, suffix and sequence bytes (FASTQ: the quality bytes are as many  */
	uint64_t suffix_bytes;      /* again); the rest are the separators                                                  */
	uint64_t seq_bytes;
	double ms_scan;             /* device time: lengths + scan; the gather                                              */
	double ms_gather;
} dbgk_fmt_info;
/* format 1 FASTQ, 2 FASTA; marker 0..255.  Anything else: DBGK_ERR_ARG.  DBGK_ERR_HIP without a usable gfx950 device: there is no
 * host fall-back                                                                                                          */
int dbgk_fmt_create(int32_t format, int32_t marker, int device, dbgk_fmt **out);
int dbgk_fmt_destroy(dbgk_fmt *f);
/* text, records, planes and offsets in device memory of f's GPU, read in place and never written; the suffix plane on the host.
 * d_text, d_bases and d_quals 16-byte aligned; d_text readable up to n_text rounded up to 16.  No source byte is read outside the
 * aligned dwords that hold a byte of a header or of a record's bytes: never at or behind n_text rounded up to 16, never behind
 * d_offsets[n] rounded up to 4; d_offsets[0] need not be 0.  DBGK_ERR_ARG with no output for: format 1 without a quality plane,
 * format 2 with one, a misaligned pointer, the stage's own output as an input, suffix offsets that do not start at 0 or decrease
 * -- and, found on the device, a header that leaves the text (head_pos + head_len > n_text), plane offsets that decrease, a record
 * of 2^32 bytes and more.  n == 0 is valid.  Work of the caller's own on the inputs has to be synchronised.  Returns when the text
 * is complete.                                                                                                            */
int dbgk_fmt_records_device(dbgk_fmt *f, const char *d_text, uint64_t n_text, const dbgk_parse_rec *d_recs, const char *d_bases,
                            const char *d_quals, const uint64_t *d_offsets, uint64_t n, const char *suffix, const uint64_t *suffix_offsets,
                            dbgk_fmt_info *out);
/* dbgk_fmt_records_device with the suffix plane in device memory of f's GPU too, read in place and never written -- what
 * dbgk_corr_annot_device returns: d_suffix 16-byte aligned with its last dword readable, d_suffix_offsets n + 1 64-bit values, both
 * null for all empty.  What dbgk_fmt_records_device checks of a suffix plane on the host is found on the device here and answered
 * with DBGK_ERR_ARG and no output (dbgk_fmt_results then gives DBGK_ERR_STATE): offsets that do not start at 0, that decrease, a total
 * of 2^32 or more -- the plane's bytes are not read before the offsets have passed.  A misaligned plane, offsets without a plane
 * that hold bytes, or the stage's own output as the plane: DBGK_ERR_ARG before any device work, as for the other inputs.      */
int dbgk_fmt_records_device_suffix(dbgk_fmt *f, const char *d_text, uint64_t n_text, const dbgk_parse_rec *d_recs, const char *d_bases,
                                   const char *d_quals, const uint64_t *d_offsets, uint64_t n, const char *d_suffix,
                                   const uint64_t *d_suffix_offsets, dbgk_fmt_info *out);
/* the same with everything on the host, uploaded by the call: offsets[n] bytes of each plane                               */
int dbgk_fmt_records(dbgk_fmt *f, const char *text, uint64_t n_text, const dbgk_parse_rec *recs, const char *bases, const char *quals,
                     const uint64_t *offsets, uint64_t n, const char *suffix, const uint64_t *suffix_offsets, dbgk_fmt_info *out);
/* host copy of the text of the last call: out_bytes bytes; a capacity below that: DBGK_ERR_ARG.  Before a successful call:
 * DBGK_ERR_STATE (also for dbgk_fmt_device).                                                                               */
int dbgk_fmt_results(dbgk_fmt *f, void *out, uint64_t capacity);
/* the text where it lies; valid until the next call or dbgk_fmt_destroy                                                    */
int dbgk_fmt_device(dbgk_fmt *f, const void **d_out, uint64_t *n_out);
/* the records of the parser's last chunk where they lie (n_records of them; the array dbgk_parse_results copies): what
 * dbgk_fmt_records_device takes beside the text that chunk was.  Before a successful chunk: DBGK_ERR_STATE.                  */
int dbgk_parse_recs_device(dbgk_parse *p, const dbgk_parse_rec **d_recs);
/* ... and the text of that chunk where it lies: the copy dbgk_parse_chunk uploaded (16-byte aligned, readable up to n_bytes
 * rounded up to 16, valid until the next chunk), or the caller's own buffer of dbgk_parse_chunk_device                     */
int dbgk_parse_text_device(dbgk_parse *p, const char **d_text, uint64_t *n_bytes);

/* ---- ROWS: from the mapper's hits to the lines of map_reads' and map_pair's output files (additions to ABI 7) ----------------------------
 * The stage behind the mapper: a batch of reads as the parser left it (the text with its records for the header lines, the bases
 * plane with its n + 1 offsets), two dbgk_map_hit per read, and a contig table of the caller's become the text the host loops of
 * bin/map_reads and bin/map_pair write for that batch, byte for byte, in up to three streams:
 *   DBGK_MAPROW_READS (map_reads.cpp; one side; hits 2 i and 2 i + 1 are alignments a and b of read i)
 *     stream 0  the 2ctg lines   row(a) "\t" row(b) "\n"        a and b on two different contigs
 *     stream 1  the 1ctg lines   row(a) "\n"                    a alone
 *     stream 2  the .reads.fa records of stream 0's reads, ">" id "\n" bases "\n"
 *     counters: total_read_num, map_ctg_diff_num, map_ctg_same_num, map_no_no_num, error_map_num (a and b on one contig: no text).
 *     A read shorter than min_read_len is neither written nor counted.
 *   DBGK_MAPROW_PAIR (map_pair.cpp; two sides; read i of side 0 and read i of side 1 are pair i, hit 2 i of each side its alignment)
 *     stream 0  the 2ctg lines   row(mate 1) "\t" row(mate 2) "\n"    two different contigs
 *     stream 1  the 1ctg lines   the same line, one contig
 *     stream 2  the gap lines    row "\n" of the one mate that is mapped
 *     counters: total_read_pair_num, map_ctg_diff_num, map_ctg_same_num, map_ctg_gap_num, map_no_no_num.  A pair with a mate shorter
 *     than min_read_len is neither written nor counted.
 * A hit is mapped when its contig is not -1.  A row is
 *   id "\t" read_len "\t" read_start "\t" read_end "\t" contig_id "\t" contig_len "\t" contig_start "\t" contig_end "\t" direct "\t" identity "%"
 * with id the first token of the header line under the handle's delimiter set, followed by "-" and the second token if there is one (a
 * header of delimiters only: empty; a '\r' the parser left in the line is a token byte), direct the low byte of the hit's field, and
 * identity the host's `ostream << (float)(1.0 - (float)mismatches / align_len) * 100`, reproduced digit for digit while it prints
 * without an exponent.  An identity below 10^-4 % (align_len near 2^24 and more) would print in exponent form: it is counted in
 * `unprintable`, and a batch that holds one writes NO text -- the counters are valid, the streams are empty and DBGK_OK is returned;
 * the caller formats that batch on the host.
 * Each stream starts on a 16-byte boundary, is written in whole 16-byte vectors with the pad of the last one 0, and 64 readable bytes
 * follow it, so dbgk_gz_deflate_device reads it where it lies.  n < 2^31, n_text < 2^31, a read below 2^31 bytes, a line below 2^32. */
typedef struct dbgk_maprow dbgk_maprow;
#define DBGK_MAPROW_READS 1
#define DBGK_MAPROW_PAIR  2
#define DBGK_MAPROW_STREAMS 3
#define DBGK_MAPROW_TILE 4096       /* bytes of output per workgroup round of the write kernel                             */
typedef struct dbgk_maprow_side {   /* one side of a batch: what the parser delivered for one file                          */
	const char *text;               /* the chunk the parser parsed, n_text bytes                                            */
	uint64_t n_text;
	const dbgk_parse_rec *recs;     /* n records, of which head_pos and head_len are used                                   */
	const char *bases;              /* the bases plane and its n + 1 offsets; PAIR prints the lengths alone and never reads */
	const uint64_t *offsets;        /* (or uploads) the plane: it may be null there                                         */
	const dbgk_map_hit *hits;       /* dbgk_maprow_rows: 2 n hits on the host; dbgk_maprow_rows_device: unused, the side's  */
} dbgk_maprow_side;                 /* hits are the ones dbgk_maprow_take_hits took                                         */
typedef struct dbgk_maprow_info {
	uint64_t n;                     /* items: reads (READS) or pairs (PAIR)                                                 */
	uint64_t counters[5];           /* the five numbers of the program's .stat file, in the order given above               */
	uint64_t stream_bytes[DBGK_MAPROW_STREAMS]; /* bytes of each stream (without the pad)                                   */
	uint64_t unprintable;           /* rows whose identity needs an exponent; not 0: no text, stream_bytes all 0            */
	double ms_scan;                 /* device time: token spans + lengths + scans; segments + the write kernels             */
	double ms_write;
} dbgk_maprow_info;
/* mode: DBGK_MAPROW_READS or DBGK_MAPROW_PAIR.  format_delims: the delimiter set of the id, 1 to 16 bytes of 1..127 (map_reads:
 * ">@ \t\n"; map_pair: "@ \t" for FASTQ, "> \t" for FASTA).  min_read_len >= 0.  Anything else: DBGK_ERR_ARG before any device work.
 * DBGK_ERR_HIP without a usable gfx950 device: there is no host fall-back                                                    */
int dbgk_maprow_create(int32_t mode, const char *format_delims, int32_t min_read_len, int device, dbgk_maprow **out);
int dbgk_maprow_destroy(dbgk_maprow *r);
/* the contig table: n ids back to back, id c = names[name_offsets[c], name_offsets[c + 1]) (name_offsets[0] == 0, non-decreasing),
 * and the length every row of contig c prints (bin/map_*: the contig's size after the short ones were emptied).  The handle is not
 * tied to a mapper's contigs.  Replaces the earlier table; n < 2^31                                                            */
int dbgk_maprow_set_contigs(dbgk_maprow *r, const char *names, const uint64_t *name_offsets, const uint32_t *lengths, uint64_t n);
/* the hits of the mapper's last batch, copied device to device into side 0 or 1 of r and ordered by events on the two streams: the
 * mapper may map its next batch at once.  Handles on different devices: DBGK_ERR_ARG; no batch mapped: DBGK_ERR_STATE          */
int dbgk_maprow_take_hits(dbgk_maprow *r, int32_t side, dbgk_map *m);
/* the rows of n items.  sides: one dbgk_maprow_side for READS, two for PAIR, every pointer in device memory of r's GPU, read in place
 * and never written; text and bases 16-byte aligned, the text readable up to n_text rounded up to 16, the plane up to offsets[n]
 * rounded up to 4.  The hits are those of dbgk_maprow_take_hits, n reads' per side (else DBGK_ERR_STATE; no contig table:
 * DBGK_ERR_STATE).  Found on the device and answered with DBGK_ERR_ARG and no output: a mapped hit whose contig is outside the table,
 * with a negative coordinate, align_len <= 0 or mismatches outside [0, align_len]; a header that leaves the text; offsets that
 * decrease.  n == 0 is valid.  Work of the caller's own on the inputs has to be synchronised.  Returns when the text is complete.  */
int dbgk_maprow_rows_device(dbgk_maprow *r, const dbgk_maprow_side *sides, uint64_t n, dbgk_maprow_info *out);
/* the same with everything on the host, the 2 n hits of each side included, uploaded by the call                            */
int dbgk_maprow_rows(dbgk_maprow *r, const dbgk_maprow_side *sides, uint64_t n, dbgk_maprow_info *out);
/* stream 0 .. 2 of the last call where it lies; valid until the next call or dbgk_maprow_destroy.  Before a successful call:
 * DBGK_ERR_STATE (also for dbgk_maprow_results)                                                                               */
int dbgk_maprow_device(dbgk_maprow *r, int32_t stream, const void **d_text, uint64_t *n_bytes);
/* host copy of a stream: stream_bytes bytes; a capacity below that: DBGK_ERR_ARG                                            */
int dbgk_maprow_results(dbgk_maprow *r, int32_t stream, void *out, uint64_t capacity);

/* ---- LINK: link_scaffold of the link_scaffold module on the GPU (additions to ABI 7) -------------------------------------------
 * link_scaffold turns the read pairs whose mates map_pair placed on two different contigs (the lines of *.map_pair.2ctg.gz) into
 * links between contigs and walks the unambiguous ones into scaffolds.  Contig c (0-based, in the order of the contig file) is node
 * 2c + 1, its reverse strand node 2c + 2 (the reference takes the node from the number in the contig's name, ctgStr2Id,
 * link_scaffold/link_func.h:130; names whose number is not 2c + 1 are undefined there and the caller's to refuse).  Every record
 * is oriented and filtered by its estimated gap (link_func.cpp:262-321 for pair ends, :367-423 for mate pairs) into two directed
 * entries; entries of one (source, target) become one link that counts and sums its first 1023 records (:458-463); a node's links
 * keep first-seen order.  That table is built on the device.  The reference's clean-up passes (remove_lowfreq_link_and_stat,
 * remove_interleaving_links, remove_repeat_nodes, remove_links_from_deleted_nodes) and its walk are serial and order-dependent
 * and run on the host, in its order (dbgk_link_resolve).  The scaffold sequences are written on the device (dbgk_link_emit).
 * Every number equals the reference's for the same records and options.                                                      */
typedef struct dbgk_link dbgk_link;

typedef struct dbgk_link_params {
	int32_t mate_pair;          /* -m IsMatePair: 0 pair ends, 1 mate pairs                                               */
	int32_t pair_num_cut;       /* -n PairNumCut, >= 0 (default 3)                                                        */
	int32_t insert_size;        /* -i InsertSize, > 0 (default 400)                                                       */
} dbgk_link_params;

/* one line of a 2ctg file as the link stage reads it */
typedef struct dbgk_link_pair {
	int32_t contig1, start1, end1;  /* mate 1: contig index, align_contig_start, align_contig_end                         */
	int32_t contig2, start2, end2;  /* mate 2                                                                             */
	uint8_t direct1, direct2;       /* 'F' / 'R'; any other byte makes the record a wrong link (a direction field of more
	                                   than one character is one as well: pass any such byte)                             */
	uint8_t pad[2];
	int32_t reserved;
} dbgk_link_pair;

typedef struct dbgk_link_entry {    /* CtgLink (link_func.h:32-37); a cleared entry is all zero                           */
	uint32_t target;
	uint32_t freq;                  /* <= 1023                                                                            */
	int64_t  size;                  /* sum of the gaps of the records counted in freq                                     */
} dbgk_link_entry;

typedef struct dbgk_link_counters { /* counted before the gap filter                                                     */
	uint64_t fr, rf, ff, rr, wrong;
} dbgk_link_counters;

/* contig >= 0: the contig, value 0 as it is, value 1 reverse-complemented (seqKmer.cpp:72-81).  contig -1: a gap of value N's.    */
typedef struct dbgk_link_item {
	int32_t contig, value;
} dbgk_link_item;

typedef struct dbgk_link_summary {
	uint64_t lowfreq;           /* LowFreq_link_num                                                                       */
	uint64_t interleave;        /* Interleave_link_num                                                                    */
	uint64_t repeat_nodes;      /* repeat_nodes_vec.size() / 2                                                            */
	uint64_t deleted;           /* Deleted_link_num                                                                       */
	uint64_t scaffolds;         /* total_scaffold_num                                                                     */
	uint64_t items;             /* contigs and gaps of all scaffolds (dbgk_link_layout)                                   */
} dbgk_link_summary;

typedef struct dbgk_link_timing {
	uint64_t records;           /* records and hit pairs added                                                            */
	uint64_t kept;              /* ... that passed the gap filter                                                         */
	uint64_t entries;           /* directed entries sorted (2 * kept)                                                     */
	uint64_t links;             /* links of the table                                                                     */
	uint64_t emit_bytes;        /* bytes the last dbgk_link_emit wrote                                                    */
	double ms_orient;           /* device time of the orient / filter kernel, summed over the batches                     */
	double ms_sort;             /* wall time of the two radix sorts (rocPRIM), their temporary buffers included           */
	double ms_reduce, ms_chain; /* device time of the capped segmented reduce and of the chain write-out                  */
	double ms_emit;             /* device time of the emit kernel of the last dbgk_link_emit                              */
} dbgk_link_timing;

/* DBGK_ERR_ARG on a bad parameter, before any device work; DBGK_ERR_HIP without a usable gfx950 device: no host fall-back  */
int dbgk_link_create(const dbgk_link_params *p, int device, dbgk_link **out);
int dbgk_link_destroy(dbgk_link *l);
/* lengths of the n_contigs contigs (each < 2^31); the link stage needs nothing else of them.  Before the first record.   */
int dbgk_link_set_contigs(dbgk_link *l, const uint32_t *lengths, uint64_t n_contigs);
/* n more records, behind those of earlier calls: record order over all calls is file order, and the table depends on it.
 * A contig index outside the contigs is DBGK_ERR_ARG.  Not after dbgk_link_build.                                         */
int dbgk_link_add_pairs(dbgk_link *l, const dbgk_link_pair *recs, uint64_t n);
/* n_pairs more records straight from the mapper: hits1[i] / hits2[i] are the first dbgk_map_hit of mate 1 / mate 2 of pair i
 * as dbgk_map_reads returned them for the same contigs.  Pairs map_pair would not have written to the 2ctg file (a mate
 * unmapped, both on one contig: map_pair.cpp:315-323) are passed over; the table equals that of dbgk_link_add_pairs on the
 * parsed text of the others.                                                                                              */
int dbgk_link_add_hits(dbgk_link *l, const dbgk_map_hit *hits1, const dbgk_map_hit *hits2, uint64_t n_pairs);
/* groups and reduces the entries on the device; once                                                                      */
int dbgk_link_build(dbgk_link *l);
/* the table: links of node i are links[first[i] .. first[i + 1]) in the order of the reference's list, i = 0 .. 2 * n_contigs
 * (first: 2 * n_contigs + 2 values).  *n_links is always set; first, links and counters may be NULL.                       */
int dbgk_link_export(dbgk_link *l, uint64_t *first, dbgk_link_entry *links, uint64_t capacity, uint64_t *n_links,
                     dbgk_link_counters *counters);
/* the reference's passes and walk over a copy of the table (the table itself stays as built)                              */
int dbgk_link_resolve(dbgk_link *l, dbgk_link_summary *out);
/* stage 0: what *.scaffold.links.all shows (after remove_lowfreq_link_and_stat), stage 1: *.scaffold.links.uniq (after every
 * pass).  inlink / link: 2 * n_contigs + 1 bytes each; links: the table's shape, cleared entries zero.  Any may be NULL.    */
int dbgk_link_snapshot(dbgk_link *l, int32_t stage, uint8_t *inlink, uint8_t *link, dbgk_link_entry *links);
/* the scaffolds in output order (by length as the reference's sort leaves them): scaffold s is items[scaf_first[s] ..
 * scaf_first[s + 1]) (summary.scaffolds + 1 and summary.items values), then the repeat contigs in output order
 * (summary.repeat_nodes values).  Scaffold ids run scf_1, scf_3, ... through the scaffolds and on through the repeats.     */
int dbgk_link_layout(dbgk_link *l, uint64_t *scaf_first, dbgk_link_item *items, int32_t *repeats);
/* scaffold read-out on the device: the items back to back into out (contig i = bases[offsets[i], offsets[i + 1]), offsets[0]
 * == 0).  *out_len is the length of the whole; DBGK_ERR_CAPACITY when capacity is below it.                                */
int dbgk_link_emit(dbgk_link *l, const char *bases, const uint64_t *offsets, uint64_t n_contigs, const dbgk_link_item *items,
                   uint64_t n_items, char *out, uint64_t capacity, uint64_t *out_len);
int dbgk_link_batch_stats(dbgk_link *l, dbgk_link_timing *out);

/* ---- FILL: link_contig of the link_scaffold module on the GPU (additions to ABI 7) ---------------------------------------------
 * link_contig links contigs by single reads whose two ends map_reads placed on two different contigs (the lines of
 * *.map_reads.2ctg.gz) and fills every gap with the consensus of the reads that span it (link_scaffold/link_contig.cpp).  The link
 * table is the LINK one without a gap filter (parse_read_ends_map_file, link_func.cpp:141-220); of the passes only
 * remove_lowfreq_link_and_stat, remove_repeat_nodes and remove_links_from_deleted_nodes run.  Per unordered contig pair the
 * records of every direction, wrong ones included, are pooled into the gap statistics (decide_gap_size, link_contig.cpp:569-610);
 * a gap of the layout whose mode is > 0 gets the per-column consensus of the reads whose own gap is the mode (:456-510), any
 * other gap cuts the left contig (:437-454).  Table, statistics, consensus and read-out are computed on the device; passes and
 * walk on the host.  Every number and byte equals the reference's for the same records, reads and options.                  */
typedef struct dbgk_fill dbgk_fill;

typedef struct dbgk_fill_params {
	int32_t pair_num_cut;       /* -n PairNumCut, >= 0 (default 3)                                                        */
	int32_t reserved[3];        /* 0                                                                                      */
} dbgk_fill_params;

/* one line of a map_reads 2ctg file as link_contig reads it; gap = align2_start - align1_end - 1 in int arithmetic */
typedef struct dbgk_fill_record {
	int32_t read;               /* index into the reads of dbgk_fill_set_reads                                            */
	int32_t read_len;           /* field 1 as written (not used by the reference either)                                  */
	int32_t align1_end;         /* field 3                                                                                */
	int32_t align2_start;       /* field 12                                                                               */
	int32_t contig1, contig2;   /* contig indices of fields 4 and 14                                                      */
	uint8_t direct1, direct2;   /* fields 8 and 18: 'F' / 'R'; any other byte makes the record a wrong link (it adds no
	                               entries to the table and still counts in the gap statistics)                           */
	uint8_t pad[2];
	int32_t reserved;
} dbgk_fill_record;

/* the statistics of one unordered contig pair (GapSize, link_contig.cpp:601-607) */
typedef struct dbgk_fill_gapstat {
	int32_t contig_lo, contig_hi;   /* contig_lo < contig_hi                                                              */
	int32_t mode;                   /* most frequent gap, the smallest one on equal frequency                             */
	int32_t mode_freq, total_freq;
	int32_t variance;               /* sum |gap - mode| * freq / total_freq, int arithmetic                               */
} dbgk_fill_gapstat;

/* contig >= 0: the first `length` bases of the contig as it is (reversed 0) or of its reverse complement (reversed 1); length is
 * the contig's unless the junction behind it cuts it.  contig -1: the junction behind a contig, gap = index into the gaps of
 * dbgk_fill_layout, length consensus bytes at cons_off of the consensus buffer (length 0 for a mode <= 0).                  */
typedef struct dbgk_fill_item {
	int32_t  contig, reversed;
	uint32_t length;
	int32_t  gap;
	uint64_t cons_off;
} dbgk_fill_item;

typedef struct dbgk_fill_gap {      /* one junction of the layout                                                         */
	int32_t mode, mode_freq, total_freq, variance;
	float   identity;               /* ConsensusSupportRate, summed in float column by column; 0 for a mode <= 0          */
	int32_t host_path;              /* 1: a spanning slice held a byte other than A C G T N, the columns were counted on
	                                   the host (same result)                                                             */
} dbgk_fill_gap;

typedef struct dbgk_fill_summary {
	uint64_t lowfreq, repeat_nodes, deleted, scaffolds, items;   /* as dbgk_link_summary                                 */
	uint64_t gaps;              /* junctions of the layout                                                                */
	uint64_t filled;            /* ... with a mode > 0                                                                    */
	uint64_t cons_bytes;        /* consensus bytes of all filled gaps                                                     */
	uint64_t pairs;             /* contig pairs with statistics                                                           */
} dbgk_fill_summary;

typedef struct dbgk_fill_timing {
	uint64_t records;           /* records and reads with hits added                                                      */
	uint64_t pooled;            /* records in the gap statistics                                                          */
	uint64_t links;
	uint64_t cons_bytes, span_bytes;   /* consensus bytes written / slice bytes read by the consensus kernel             */
	uint64_t emit_bytes;
	double ms_orient;           /* device time of the orient kernel, summed over the batches                              */
	double ms_sort;             /* wall time of all radix sorts (table and statistics)                                    */
	double ms_table;            /* device time of reduce and chain                                                        */
	double ms_gapstat;          /* device time of the gather and run-length / segmented-reduce kernels                    */
	double ms_consensus;        /* device time of the consensus kernel                                                    */
	double ms_emit;             /* device time of the emit kernel of the last dbgk_fill_emit                              */
} dbgk_fill_timing;

/* DBGK_ERR_ARG on a bad parameter, before any device work; DBGK_ERR_HIP without a usable gfx950 device: no host fall-back  */
int dbgk_fill_create(const dbgk_fill_params *p, int device, dbgk_fill **out);
int dbgk_fill_destroy(dbgk_fill *f);
int dbgk_fill_set_contigs(dbgk_fill *f, const uint32_t *lengths, uint64_t n_contigs);
/* the reads the records point into, read i = bases[offsets[i], offsets[i + 1]) (offsets[0] == 0); before dbgk_fill_resolve */
int dbgk_fill_set_reads(dbgk_fill *f, const char *bases, const uint64_t *offsets, uint64_t n_reads);
/* n more records behind those of earlier calls (record order over all calls is file order).  A contig index outside the contigs,
 * contig1 == contig2 or a negative read index is DBGK_ERR_ARG.  Not after dbgk_fill_build.                                */
int dbgk_fill_add_records(dbgk_fill *f, const dbgk_fill_record *recs, uint64_t n);
/* n_reads more records straight from the mapper: hits[2 i], hits[2 i + 1] as dbgk_map_reads (second_alignment) returned them for
 * read first_read + i of dbgk_fill_set_reads.  Reads map_reads would not have written to the 2ctg file (a hit with contig -1, both
 * on one contig: map_reads.cpp:59-73) are passed over; table and statistics equal those of the parsed text of the others.   */
int dbgk_fill_add_hits(dbgk_fill *f, const dbgk_map_hit *hits, uint64_t n_reads, uint64_t first_read);
/* the link table and the gap statistics, on the device; once */
int dbgk_fill_build(dbgk_fill *f);
/* as dbgk_link_export */
int dbgk_fill_export(dbgk_fill *f, uint64_t *first, dbgk_link_entry *links, uint64_t capacity, uint64_t *n_links,
                     dbgk_link_counters *counters);
/* the statistics of every contig pair with a record, ascending by (contig_lo, contig_hi).  *n_pairs is always set.          */
int dbgk_fill_gap_stats(dbgk_fill *f, dbgk_fill_gapstat *out, uint64_t capacity, uint64_t *n_pairs);
/* passes, walk, layout and the consensus of every filled gap.  A spanning read whose slice [align1_end, align1_end + gap) does
 * not lie inside its read is DBGK_ERR_ARG (undefined in the reference); no byte of that gap is read on the device.          */
int dbgk_fill_resolve(dbgk_fill *f, dbgk_fill_summary *out);
/* as dbgk_link_snapshot: stage 0 *.contig_R.links.all, stage 1 *.contig_R.links.uniq */
int dbgk_fill_snapshot(dbgk_fill *f, int32_t stage, uint8_t *inlink, uint8_t *link, dbgk_link_entry *links);
/* scafftigs in output order: scaf_first (summary.scaffolds + 1), items (summary.items), gaps (summary.gaps), repeat contigs
 * (summary.repeat_nodes), consensus (summary.cons_bytes bytes, copied from the device buffer).  Any may be NULL.  Ids run
 * sct_1, sct_3, ... through the scafftigs and on through the repeats.                                                     */
int dbgk_fill_layout(dbgk_fill *f, uint64_t *scaf_first, dbgk_fill_item *items, dbgk_fill_gap *gaps, int32_t *repeats, char *consensus);
/* read-out on the device: the items back to back into out; gap items take their bytes from the consensus buffer of
 * dbgk_fill_resolve on the device.  *out_len is the length of the whole; DBGK_ERR_CAPACITY when capacity is below it.      */
int dbgk_fill_emit(dbgk_fill *f, const char *bases, const uint64_t *offsets, uint64_t n_contigs, const dbgk_fill_item *items,
                   uint64_t n_items, char *out, uint64_t capacity, uint64_t *out_len);
int dbgk_fill_batch_stats(dbgk_fill *f, dbgk_fill_timing *out);

/* ---- SUPER: link_supertig of the link_scaffold module on the GPU (additions to ABI 7) ------------------------------------------
 * link_supertig links contigs or scafftigs by long reads whose two ends map_reads placed on two different sequences, writes every
 * gap as N x the mean gap and lists, per gap, the slices of the reads that span it (link_scaffold/link_supertig.cpp).  The link
 * table is FILL's; the passes are LINK's with the interleaving pass on.  Per unordered contig pair the records of every
 * direction, wrong ones included, are pooled into mean, min, max, total and mean deviation (decide_gap_size, :561-605).  Per
 * junction of the layout every record of its pair gives one slice of its read (:443-467); the slices are sorted by length with
 * the reference's std::sort, the one at index n / 2 is the median, the others are kept when their length lies strictly inside
 * 0.75 .. 1.25 x the median's (:469-495).  Table, statistics, slices and read-out are computed on the device; passes, walk and
 * slice geometry on the host.  Every number and byte equals the reference's for the same records, reads and options.         */
typedef struct dbgk_super dbgk_super;

typedef struct dbgk_super_params {
	int32_t pair_num_cut;       /* -n PairNumCut, >= 0 (default 3)                                                        */
	int32_t reserved[3];        /* 0                                                                                      */
} dbgk_super_params;

/* the statistics of one unordered contig pair (GapSize, link_supertig.cpp:595-602) */
typedef struct dbgk_super_gapstat {
	int32_t contig_lo, contig_hi;   /* contig_lo < contig_hi                                                              */
	int32_t mean;                   /* sum of the gaps / total, truncated toward zero                                     */
	int32_t min, max, total;
	int32_t variance;               /* sum |mean - gap| / total, truncated                                                */
	int32_t reserved;
} dbgk_super_gapstat;

/* one junction of the layout: the statistics as *.supertig.pos.tab prints them, and its slices */
typedef struct dbgk_super_junction {
	int32_t left_contig, right_contig;
	int32_t mean, min, max, total, variance;
	int32_t n_written;              /* N's written: mean, or 1 for a mean <= 0                                            */
	int32_t gap_id;                 /* 1, 2, ... in walk order: the id of *.supertig.gap.data and of the pos.tab line      */
	int32_t median;                 /* index of the median among the junction's slices                                    */
	uint64_t first_slice;           /* its slices are dbgk_super_slices [first_slice, first_slice + n_slices)             */
	uint32_t n_slices;
	uint32_t n_kept;                /* ... of which the median and n_kept - 1 others are written                          */
} dbgk_super_junction;

/* one slice; those of a junction come in the order the reference's sort by length leaves them */
typedef struct dbgk_super_slice {
	uint64_t record;                /* the record it comes from, counted over all dbgk_super_add_* calls                  */
	uint64_t offset;                /* kept != 0: its bytes begin here in the slice bytes                                 */
	uint32_t length;
	uint8_t  reversed;              /* 1: the reverse complement of the read's bytes                                      */
	uint8_t  kept;                  /* 2: the median (line Y), 1: written (line N), 0: dropped (Altert message)           */
	uint8_t  pad[2];
} dbgk_super_slice;

typedef struct dbgk_super_summary {
	uint64_t lowfreq, interleave, repeat_nodes, deleted, scaffolds, items;   /* as dbgk_link_summary                     */
	uint64_t junctions;         /* junctions of the layout                                                                */
	uint64_t slices;            /* slices of all junctions                                                                */
	uint64_t lines;             /* ... that are written: the S ids of *.supertig.gap.data run 1 .. lines                  */
	uint64_t slice_bytes;       /* bytes of the written slices                                                            */
	uint64_t pairs;             /* contig pairs with statistics                                                           */
	int64_t  bad_record;        /* DBGK_ERR_ARG from dbgk_super_resolve: the record whose slice does not lie in its read  */
	int64_t  bad_read;          /* ... its read, and the junction's two contigs; -1 otherwise                             */
	int32_t  bad_left, bad_right;
} dbgk_super_summary;

typedef struct dbgk_super_timing {
	uint64_t records;           /* records and reads with hits added                                                      */
	uint64_t pooled;            /* records in the gap statistics                                                          */
	uint64_t links;
	uint64_t slice_bytes;       /* bytes the slice kernel wrote (it read as many)                                         */
	uint64_t emit_bytes;
	double ms_orient;           /* device time of the orient kernel, summed over the batches                              */
	double ms_sort;             /* wall time of all radix sorts (table and statistics)                                    */
	double ms_table;            /* device time of reduce and chain                                                        */
	double ms_gapstat;          /* device time of the two segmented-reduce passes and the pack kernel                     */
	double ms_slices;           /* device time of the slice kernel                                                        */
	double ms_emit;             /* device time of the emit kernel of the last dbgk_super_emit                             */
} dbgk_super_timing;

/* DBGK_ERR_ARG on a bad parameter, before any device work; DBGK_ERR_HIP without a usable gfx950 device: no host fall-back  */
int dbgk_super_create(const dbgk_super_params *p, int device, dbgk_super **out);
int dbgk_super_destroy(dbgk_super *s);
int dbgk_super_set_contigs(dbgk_super *s, const uint32_t *lengths, uint64_t n_contigs);
/* the reads the records point into, as dbgk_fill_set_reads; before dbgk_super_resolve.  A record may name a read index at or
 * above n_reads (a read missing from the reads files): it counts in table and statistics and fails the junction it spans.  */
int dbgk_super_set_reads(dbgk_super *s, const char *bases, const uint64_t *offsets, uint64_t n_reads);
/* as dbgk_fill_add_records: the same fields of the same line */
int dbgk_super_add_records(dbgk_super *s, const dbgk_fill_record *recs, uint64_t n);
/* as dbgk_fill_add_hits */
int dbgk_super_add_hits(dbgk_super *s, const dbgk_map_hit *hits, uint64_t n_reads, uint64_t first_read);
/* the link table and the gap statistics, on the device; once.  A pair whose gap sum or deviation sum leaves int32 (undefined in
 * the reference) is DBGK_ERR_ARG.                                                                                          */
int dbgk_super_build(dbgk_super *s);
/* as dbgk_link_export */
int dbgk_super_export(dbgk_super *s, uint64_t *first, dbgk_link_entry *links, uint64_t capacity, uint64_t *n_links,
                      dbgk_link_counters *counters);
/* the statistics of every contig pair with a record, ascending by (contig_lo, contig_hi).  *n_pairs is always set.          */
int dbgk_super_gap_stats(dbgk_super *s, dbgk_super_gapstat *out, uint64_t capacity, uint64_t *n_pairs);
/* passes, walk, layout and the slices of every junction.  A slice that begins before its read's first byte or behind its last one,
 * or a read index outside the reads (the reference throws out of substr), is DBGK_ERR_ARG with out->bad_* set; no byte of
 * that junction is read on the device.                                                                                    */
int dbgk_super_resolve(dbgk_super *s, dbgk_super_summary *out);
/* as dbgk_link_snapshot: stage 0 *.supertig.links.all, stage 1 *.supertig.links.uniq */
int dbgk_super_snapshot(dbgk_super *s, int32_t stage, uint8_t *inlink, uint8_t *link, dbgk_link_entry *links);
/* super-contigs in output order: scaf_first (summary.scaffolds + 1), items (summary.items; the gap behind a contig is an item of
 * n_written N's), junctions (summary.junctions, in the order of the gap items), repeat contigs (summary.repeat_nodes).  Any
 * may be NULL.  Ids run spt_1, spt_3, ... through the super-contigs and on through the repeats.                            */
int dbgk_super_layout(dbgk_super *s, uint64_t *scaf_first, dbgk_link_item *items, dbgk_super_junction *junctions, int32_t *repeats);
/* the slices of all junctions, those of gap_id 1 first.  *n_slices is always set.                                          */
int dbgk_super_slices(dbgk_super *s, dbgk_super_slice *out, uint64_t capacity, uint64_t *n_slices);
/* the bytes of the written slices back to back in the order *.supertig.gap.data lists them (per junction the median, then the
 * others as sorted), copied from the device buffer.  *n_bytes is always set.                                               */
int dbgk_super_slice_bytes(dbgk_super *s, char *out, uint64_t capacity, uint64_t *n_bytes);
/* as dbgk_link_emit */
int dbgk_super_emit(dbgk_super *s, const char *bases, const uint64_t *offsets, uint64_t n_contigs, const dbgk_link_item *items,
                    uint64_t n_items, char *out, uint64_t capacity, uint64_t *out_len);
int dbgk_super_batch_stats(dbgk_super *s, dbgk_super_timing *out);

/* ---- CONTIG: the contig read-out of debruijn_contig on the GPU (additions to ABI 7) ---------------------------------------------
 * read_out_contig (DBG_contig/contig.cpp:900-1011) scans the simplified table in slot order; at the first live linear node it
 * walks right, then left (get_linear_seq, :832-896), deletes what it passes and stops at the first neighbour that is not linear or
 * not there.  Here every live linear node finds its two successors on the device (the probe of exist_kmerset, kmerSet.cpp:280-302,
 * on the host-layout table), chains whose every step is answered by the neighbour's link back are ranked by pointer jumping from
 * their smallest slot -- where the reference's scan starts them -- and written out on the device; every other chain (a step that
 * is not answered, a step of a node onto itself, a cycle) is walked on the host in ascending slot order, as the reference does.
 * The handle takes the table as the host holds it after simplification and no graph handle.  Contigs come in the order the
 * reference's scan finds them; sorting, ids and the -M split are the caller's.  Every byte equals the reference's.             */
typedef struct dbgk_contig dbgk_contig;

typedef struct dbgk_contig_params {
	int32_t k;                  /* 1 .. 31; 1 .. 63 for dbgk_wide_contig_create                                           */
	int32_t kmer_freq_cutoff;   /* -D, as the klink records were computed with; kept for the record, the read-out reads klink */
	int32_t contig_len_cutoff;  /* -M; kept for the record: the split into contigs and small ones is the caller's         */
	int32_t reserved;           /* 0                                                                                      */
} dbgk_contig_params;

/* one contig: bytes left_len (reversed left walk) + k (the anchor's k-mer) + right_len (right walk) */
typedef struct dbgk_contig_record {
	uint64_t anchor;                    /* the slot the walks start from                                                  */
	uint64_t left_end, right_end;       /* the slot a walk stopped at; the table size when there was no such node         */
	uint32_t left_len, right_len;       /* steps of either walk (contig_leftward_len, contig_rightward_len)               */
	uint32_t left_depth, right_depth;   /* sums of the steps' link depths                                                 */
	uint8_t  left_mark, right_mark;     /* 0 break, 1 branch                                                              */
	uint8_t  left_repeat, right_repeat; /* 0 Unknown, 1 Unique, 2 Repeat                                                  */
	uint8_t  host_walked;               /* 1: read out by the host walker                                                 */
	uint8_t  mid_depth;                 /* the depth byte of the k-mer's k bases: (char)avgDepth, 10 and 62 one less      */
	uint8_t  pad[2];
} dbgk_contig_record;

typedef struct dbgk_contig_summary {
	uint64_t contigs;           /* all, = kernel_contigs + host_contigs                                                   */
	uint64_t kernel_contigs;    /* read out by the kernels                                                                */
	uint64_t host_contigs;      /* read out by the host walker                                                            */
	uint64_t bytes;             /* bases of all contigs (as many depth bytes)                                             */
	uint64_t linear_nodes;      /* live linear nodes of the table                                                         */
	uint64_t host_nodes;        /* ... on chains handed to the host walker                                                */
	uint64_t rounds;            /* pointer-jumping rounds                                                                 */
	uint64_t reserved;
} dbgk_contig_summary;

typedef struct dbgk_contig_timing {
	uint64_t upload_bytes;      /* table, flags and link records copied to the device by dbgk_contig_set_table            */
	uint64_t emit_bytes;        /* bytes the emit kernel wrote (bases + depths)                                           */
	double ms_upload;           /* wall time of that copy                                                                 */
	double ms_compact;          /* device time: numbering the live linear nodes (two kernels)                             */
	double ms_successors;       /* device time of the successor kernel                                                    */
	double ms_mutual;           /* device time of the order-independence check and the initial port states                */
	double ms_rank;             /* device time of all pointer-jumping rounds                                              */
	double ms_place;            /* device time: classify, contig numbering and offsets                                    */
	double ms_scatter;          /* device time of the scatter of the steps                                                */
	double ms_emit;             /* device time of the emit kernel                                                         */
	double ms_host_walk;        /* wall time of the host walker                                                           */
} dbgk_contig_timing;

/* DBGK_ERR_ARG on a bad parameter, before any device work; DBGK_ERR_HIP without a usable gfx950 device: no host fall-back  */
int dbgk_contig_create(const dbgk_contig_params *p, int device, dbgk_contig **out);
int dbgk_contig_destroy(dbgk_contig *c);
/* the table after simplification, as the host holds it: array[size], nul_flag and del_flag of size / 8 + 1 bytes (kmerSet.h:144-169),
 * klink[size] in the layout of dbgk_export_host_table_links (byte 1 bit 0 = linear).  2 <= size < 2^32 - 1.  Copied to the device;
 * the host arrays are read again by dbgk_contig_read_out (host walker) and must stay as they are until it returns.             */
int dbgk_contig_set_table(dbgk_contig *c, uint64_t size, const dbgk_node *array, const uint8_t *nul_flag, const uint8_t *del_flag,
                          const uint16_t *klink);
/* the read-out; neither the host arrays nor their device copies are changed.  out may be NULL.  More than 2^30 - 1 live linear
 * nodes are DBGK_ERR_ARG.                                                                                                     */
int dbgk_contig_read_out(dbgk_contig *c, dbgk_contig_summary *out);
int dbgk_contig_summary_get(dbgk_contig *c, dbgk_contig_summary *out);
/* contigs in the order of the reference's scan: offsets (summary.contigs + 1; contig i is bytes [offsets[i], offsets[i + 1]) of
 * bases and of depths), records (summary.contigs), bases and depths (summary.bytes each).  Any may be NULL.                   */
int dbgk_contig_results(dbgk_contig *c, uint64_t *offsets, dbgk_contig_record *records, char *bases, char *depths);
int dbgk_contig_timing_get(dbgk_contig *c, dbgk_contig_timing *out);

/* ---- CONTIG on 128-bit keys (additions to ABI 7; this build only: PARITY UNPINNED above k = 32) -------------------------------------
 * The same read-out for a table of dbgk_node32 (include/dbgk_wide.h), k = 1 .. 63.  The reference stops at k = 31, so nothing pins
 * the bytes above k = 32; the rules are those of dbgk_wide.h (revcomp, 128-bit comparison, hash_code(lo ^ hash_code(hi)) for a high
 * word that is not 0, linear probing with wrap), every one of which is the reference's 64-bit rule when the high word is 0: a wide
 * handle at k <= 31 on a table of {0, kmer} nodes returns what a handle of dbgk_contig_create returns for the 16-byte table.
 * dbgk_contig_read_out, _results, _summary_get, _timing_get and _destroy serve both kinds of handle; slots stay 32-bit, so records,
 * summary and timing are the same structs.  k outside 1 .. 63 is DBGK_ERR_ARG before any device work; DBGK_ERR_HIP without a usable
 * gfx950 device: no host fall-back.                                                                                              */
int dbgk_wide_contig_create(const dbgk_contig_params *p, int device, dbgk_contig **out);
/* as dbgk_contig_set_table, 32-byte nodes; the same flag and link-record layouts, 2 <= size < 2^32 - 1.  On a handle of
 * dbgk_contig_create this is DBGK_ERR_STATE, as dbgk_contig_set_table is on a handle of dbgk_wide_contig_create.                  */
int dbgk_wide_contig_set_table(dbgk_contig *c, uint64_t size, const dbgk_node32 *array, const uint8_t *nul_flag, const uint8_t *del_flag,
                               const uint16_t *klink);

/* ---- SIMPLIFY: the linear paths of the contig stage's simplification passes, traced on the GPU (additions to ABI 7) ------------------
 * remove_error_tips, remove_lowCov_edges and remove_hetero_bubbles (DBG_contig/contig.cpp:281-776) call get_linear_path (:779-827) once
 * per list entry, in list order.  These calls trace all walks of a pass at once on the device copy of the table a CONTIG handle holds
 * (dbgk_contig_set_table / dbgk_wide_contig_set_table), as the table stands at that moment; the caller consumes them in list order and
 * walks a path itself where a trace touches a slot it has changed since.  dbgk_simplify_update carries the caller's changes into the
 * device copy.  All calls serve both kinds of handle (PARITY UNPINNED above k = 32, as for the read-out).  Arguments are checked before
 * any device work: a slot at or above the table size, a direct other than +1 / -1 and a len_cutoff above DBGK_TRACE_MAX_CUTOFF are
 * DBGK_ERR_ARG, a call before set_table is DBGK_ERR_STATE.  There is no host fall-back.                                              */
#define DBGK_TRACE_MAX_CUTOFF 65536   /* a walk on a cycle ends at the cutoff only */

typedef struct dbgk_trace_request {
	uint64_t slot;              /* the node the walk starts from: walked whatever its state                                */
	int32_t  direct;            /* +1 leaving rightward, -1 leaving leftward                                              */
	int32_t  reserved;          /* 0                                                                                      */
} dbgk_trace_request;

/* status of a row */
#define DBGK_TRACE_TRACED        0   /* a walk: len >= 1                                                                   */
#define DBGK_TRACE_BELOW_CUTOFF  1   /* branch rows: the edge's depth is not above kmer_freq_cutoff; no neighbour looked up */
#define DBGK_TRACE_ABSENT        2   /* branch rows: the neighbour is not in the table (or deleted); start = table size    */
#define DBGK_TRACE_NOT_LINEAR    3   /* branch rows: the neighbour (start) is no linear node                               */

typedef struct dbgk_trace_row {
	uint32_t start;             /* slot the walk starts from; table size when there is none                               */
	uint32_t last;              /* the slot get_linear_path returns; table size when there is no such node                */
	uint32_t len;               /* steps (0 without a walk)                                                               */
	uint32_t depth;             /* sum of the steps' link depths                                                          */
	int8_t   direct;            /* direction at start, +1 / -1 (for a branch row: after the flip); 0 when not looked up   */
	uint8_t  mark;              /* 0 break, 1 branch                                                                      */
	uint8_t  status;            /* DBGK_TRACE_*                                                                           */
	uint8_t  pad;
	uint32_t reserved;
} dbgk_trace_row;

typedef struct dbgk_trace_summary {
	uint64_t rows;              /* requests, or 8 per branching slot                                                      */
	uint64_t traced;            /* rows with a walk                                                                       */
	uint64_t nodes;             /* steps of all walks                                                                     */
	uint64_t batches;           /* batches the rows were traced in                                                        */
} dbgk_trace_summary;

typedef struct dbgk_simplify_timing {   /* sums since set_table */
	uint64_t bytes_returned;    /* rows, nodes and base codes copied back from the device                                 */
	uint64_t batches;
	uint64_t updated_slots;
	uint64_t reserved;
	double ms_trace;            /* device time of the length pass of dbgk_simplify_trace                                  */
	double ms_branches;         /* ... of dbgk_simplify_trace_branches                                                    */
	double ms_fill;             /* device time of the pass that writes nodes and base codes                               */
	double ms_update;           /* device time of the update kernel                                                       */
} dbgk_simplify_timing;

/* get_linear_path(req[i].slot, req[i].direct, len_cutoff) for every i < n, one row each.  out may be NULL; n may be 0.           */
int dbgk_simplify_trace(dbgk_contig *c, const dbgk_trace_request *req, uint64_t n, int32_t len_cutoff, dbgk_trace_summary *out);
/* for every listed slot 8 rows: row 8 i + 4 side + j is the edge of base j on the right (side 0) or left (side 1) of slots[i].  An edge
 * whose link depth is above the handle's kmer_freq_cutoff (get_branch_bases, :361-370) has its neighbour looked up; a neighbour that is
 * a live linear node is traced with len_cutoff, in the direction the walk has there.                                               */
int dbgk_simplify_trace_branches(dbgk_contig *c, const uint64_t *slots, uint64_t n, int32_t len_cutoff, dbgk_trace_summary *out);
/* what the last trace call found: rows (summary.rows), node_offsets (rows + 1: row i's steps are [node_offsets[i], node_offsets[i + 1])
 * of nodes and of bases), nodes (summary.nodes slots), bases (summary.nodes base codes 0..3 = ACGT, in the orientation the path's
 * string has, :793-800).  Any pointer may be NULL.  DBGK_ERR_STATE before a trace call.                                             */
int dbgk_simplify_trace_results(dbgk_contig *c, dbgk_trace_row *rows, uint64_t *node_offsets, uint32_t *nodes, uint8_t *bases);
/* reads the host arrays given to set_table again at these slots -- the node's two link words, its link record, its delete bit -- and
 * writes them into the device copy.  A slot may be listed more than once.                                                          */
int dbgk_simplify_update(dbgk_contig *c, const uint64_t *slots, uint64_t n);
int dbgk_simplify_timing_get(dbgk_contig *c, dbgk_simplify_timing *out);

/* the global alignments of remove_hetero_bubbles (DBG_contig/contig.cpp:375-582), many independent pairs at once: what global_aligning
 * (DBG_contig/global_aligning.cpp:98-182) returns for each pair, bit for bit -- match 3, mismatch -5, gap -5, the tie rule of get_max_score
 * (:20-35), trace_back (:39-68).  An alignment depends on its two strings only, so the calls work on a CONTIG handle of either kind, with
 * or without a table, and use its device and stream alone.  Checked before any device work: a sequence of length 0, a byte other than
 * A C G T and decreasing offsets are DBGK_ERR_ARG; dbgk_align_results before any dbgk_align_pairs is DBGK_ERR_STATE.  n_pairs == 0 touches
 * no device.  A pair with a sequence longer than DBGK_ALIGN_MAX_LEN is not aligned: it comes back DBGK_ALIGN_TOO_LONG and the caller
 * aligns it itself.  There is no host fall-back.  (The three calls do not carry the section's dbgk_simplify_ prefix: the set of symbols
 * with that prefix is pinned where the trace calls are tested.)                                                                      */
#define DBGK_ALIGN_MAX_LEN   256     /* covers -U up to 193 at k = 63 */
#define DBGK_ALIGN_DONE      0
#define DBGK_ALIGN_TOO_LONG  1

typedef struct dbgk_align_row {     /* one per pair */
	uint32_t len_i, len_j;
	int32_t  score;             /* DPscore[len_i][len_j]; 0 when TOO_LONG                                                 */
	uint32_t aligned_len;       /* columns of the alignment; 0 when TOO_LONG                                              */
	uint32_t diffs;             /* columns that compare_two_seq_simple (contig.cpp:587-595) counts: two different letters; a
	                             * column with a gap does not count.  0 when TOO_LONG                                     */
	uint8_t  status, pad[3];    /* DBGK_ALIGN_*                                                                           */
} dbgk_align_row;

typedef struct dbgk_align_summary {
	uint64_t pairs;             /* = aligned + too_long                                                                   */
	uint64_t aligned, too_long;
	uint64_t batches;           /* kernel launches the pairs went through                                                 */
	uint64_t aligned_bytes;     /* columns of all alignments: bytes of aligned_i, and of aligned_j                        */
	uint64_t reserved;
} dbgk_align_summary;

typedef struct dbgk_align_timing {  /* sums since create */
	uint64_t bytes_up;          /* sequences and offsets copied to the device                                             */
	uint64_t bytes_back;        /* rows and aligned strings copied back                                                   */
	uint64_t batches, pairs;    /* kernel launches; pairs aligned by them                                                 */
	uint64_t cells;             /* len_i x len_j over those pairs                                                         */
	uint64_t reserved;
	double ms_align;            /* device time of the kernel                                                              */
} dbgk_align_timing;

/* pair p = sequences 2 p and 2 p + 1 of `seqs`: sequence s is bytes [offsets[s], offsets[s + 1]); offsets has 2 n_pairs + 1 entries.
 * out may be NULL.                                                                                                             */
int dbgk_align_pairs(dbgk_contig *c, const char *seqs, const uint64_t *offsets, uint64_t n_pairs, dbgk_align_summary *out);
/* what the last dbgk_align_pairs found: rows (n_pairs); aligned_offsets (n_pairs + 1, in columns: pair p's two aligned strings are
 * bytes [aligned_offsets[p], aligned_offsets[p + 1]) of aligned_i and of aligned_j).  Any pointer may be NULL.                     */
int dbgk_align_results(dbgk_contig *c, dbgk_align_row *rows, uint64_t *aligned_offsets, char *aligned_i, char *aligned_j);
int dbgk_align_timing_get(dbgk_contig *c, dbgk_align_timing *out);

/* ---- which level-1 kernels ran (additions to ABI 7) ---------------------------------------------
 * The level-1 kernel forms that the batches of a PARTITION / WIDE record handle launched since the last dbgk_reset or
 * dbgk_reset_timings, in launch order: one line per launch, "family=... wide_d=... ... dbg=0\n", the text the library's
 * own error messages use for a form.  The handle keeps the first 16 launches; *n_launches (may be NULL) gets the number
 * of all of them.  buf gets a terminated string; DBGK_ERR_ARG if cap is too small for it (4096 bytes always suffice).  */
int dbgk_l1_forms_text(dbgk_handle *h, char *buf, size_t cap, uint32_t *n_launches);

int dbgk_device_count(void);
int dbgk_abi_version(void);
const char *dbgk_strerror(int status);
/* text of the most recent HIP failure seen by this thread ("" if none) */
const char *dbgk_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DBGK_H_ */
