"""ctypes binding of the C ABI in include/dbgk.h (dbg_assembly_amd/lib/libdbgk.so).

Plumbing only: every compute call goes straight into the HIP library.  There is no Python or CPU
fallback -- loading fails loudly if the library has not been built, and dbgk_create fails if no
gfx950 device is present.
"""
import collections
import ctypes as C
import os

import numpy as np

# ONE HIP runtime per process.  torch ships its own libamdhip64 / libhsa-runtime64; if libdbgk.so (linked against /opt/rocm) is
# loaded FIRST, both copies end up in the process and torch's finds no device ("No HIP GPUs are available").  With torch's loaded
# first the library binds to that copy (same soname) and everything -- zero-copy tensors over the library's buffers, pinned
# tensors recognised by dbgk_push_reads -- shares one runtime (profiles/ubench/hip_runtime_order.py shows both orders).  A C++
# caller never sees this; it only concerns Python processes that use both.
try:
    import torch  # noqa: F401  (plumbing: load order only)
except ImportError:
    pass

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DBGK_LIB") or os.path.join(HERE, "lib", "libdbgk.so")  # DBGK_LIB: A/B runs of two builds in one session

NODE_DTYPE = np.dtype([("kmer", "<u8"), ("l_link", "<u4"), ("r_link", "<u4")])
NODE32_DTYPE = np.dtype([("kmer_hi", "<u8"), ("kmer_lo", "<u8"), ("l_link", "<u4"), ("r_link", "<u4"), ("reserved", "<u8")])  # dbgk_node32

OK, ERR_ARG, ERR_HIP, ERR_TABLE_FULL, ERR_STATE, ERR_NOMEM, ERR_CAPACITY = 0, -1, -2, -3, -4, -5, -6
ENGINE_AUTO, ENGINE_DIRECT, ENGINE_PARTITION, ENGINE_KFREQ, ENGINE_SEEDIDX, ENGINE_WIDE = 0, 1, 2, 3, 4, 5
FLAG_TRACK_FIRST_SEEN = 1
FLAG_PREALLOC_STAGING = 2


class SynthParams(C.Structure):
    _fields_ = [("genome_len", C.c_uint64), ("read_len", C.c_uint32), ("sub_thr", C.c_uint32),
                ("n_thr", C.c_uint32), ("reserved", C.c_uint32), ("genome_seed", C.c_uint64),
                ("read_seed", C.c_uint64), ("err_seed", C.c_uint64)]


def synth_params(genome_len, read_len=150, sub_rate=0.005, n_rate=0.0001, cfg=2):
    """SURVEY.md section 8(d) seeds: genome 0xD8B6A55E0000+cfg, reads 0x5EED0000+cfg."""
    return SynthParams(genome_len, read_len, int(round(sub_rate * 2 ** 32)), int(round(n_rate * 2 ** 24)), 0,
                       0xD8B6A55E0000 + cfg, 0x5EED0000 + cfg, 0xE4404000 + cfg)


class Config(C.Structure):
    _fields_ = [("kmer_size", C.c_int32), ("max_read_len", C.c_int32), ("table_slots", C.c_uint64),
                ("device_id", C.c_int32), ("engine", C.c_int32), ("max_batch_bases", C.c_uint64),
                ("expected_kmers", C.c_uint64), ("shard_count", C.c_uint32), ("shard_index", C.c_uint32),
                ("flags", C.c_uint64), ("n_passes", C.c_uint64), ("reserved", C.c_uint64 * 1)]


class ShardInfo(C.Structure):
    _fields_ = [("n_ranks", C.c_uint32), ("rank", C.c_uint32), ("table_slots_global", C.c_uint64),
                ("slot_lo", C.c_uint64), ("slot_hi", C.c_uint64), ("d_send", C.c_void_p), ("d_recv", C.c_void_p),
                ("chunk_bytes", C.c_uint64), ("d_send_cnt", C.c_void_p), ("d_recv_cnt", C.c_void_p),
                ("cnt_chunk_bytes", C.c_uint64), ("buckets_per_rank", C.c_uint32), ("own_buckets", C.c_uint32),
                ("bucket_bytes", C.c_uint64), ("cnt_bucket_bytes", C.c_uint64)]


class PlanInfo(C.Structure):
    _fields_ = [("table_slots", C.c_uint64), ("r", C.c_uint32), ("level1_buckets", C.c_uint32), ("final_per_level1", C.c_uint32),
                ("three_level", C.c_uint32), ("buckets_per_rank", C.c_uint32), ("own_buckets", C.c_uint32), ("first_bucket", C.c_uint32),
                ("reserved", C.c_uint32), ("slot_lo", C.c_uint64), ("slot_hi", C.c_uint64), ("records_per_level1_bucket", C.c_uint64),
                ("records_per_final_bucket", C.c_uint64), ("table_bytes", C.c_uint64), ("level1_store_bytes", C.c_uint64),
                ("inbox_bytes", C.c_uint64), ("final_store_bytes", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("total_reads", C.c_uint64), ("total_kmers", C.c_uint64), ("stored_kmers", C.c_uint64),
                ("count", C.c_uint64), ("count_conflict", C.c_uint64), ("table_slots", C.c_uint64),
                ("polyA_l_link", C.c_uint32), ("polyA_r_link", C.c_uint32), ("other_bytes", C.c_uint64)]


class LinkStats(C.Structure):
    _fields_ = [("depth_stat", C.c_int64 * 256), ("total_nodes", C.c_int64), ("deleted_lowfreq", C.c_int64),
                ("linear_nodes", C.c_int64), ("tip_nodes", C.c_int64), ("branch_nodes", C.c_int64)]


class Timings(C.Structure):
    _fields_ = [("mark_ms", C.c_float), ("insert_ms", C.c_float), ("partition_ms", C.c_float),
                ("build_ms", C.c_float), ("fixup_ms", C.c_float), ("finalize_ms", C.c_float),
                ("insert_launches", C.c_uint64), ("l2_build_wall_ms", C.c_float), ("partition_launches", C.c_uint32),
                ("uniform_launches", C.c_uint32), ("prefix_launches", C.c_uint32), ("reserved", C.c_uint64 * 1)]


class CorrParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("min_high_region", C.c_int32), ("max_change", C.c_int32), ("further_trim", C.c_int32),
                ("max_tree_nodes", C.c_int32), ("min_trimmed_len", C.c_int32)]


CORR_REC_DTYPE = np.dtype([("one_base", "<u4"), ("tree", "<u4"), ("left_trim", "<u4"), ("right_trim", "<u4"),
                           ("node_limit_hits", "<u4"), ("deleted", "u1"), ("path", "u1"), ("pad", "u1", (2,))])  # dbgk_corr_rec


class CorrStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("by_classify", C.c_uint64), ("by_correct", C.c_uint64), ("by_overflow", C.c_uint64),
                ("node_limit_hits", C.c_uint64), ("ms_classify", C.c_double), ("ms_correct", C.c_double),
                ("ms_overflow", C.c_double)]


CORR_COMPACT_TILE = 4096  # DBGK_CORR_COMPACT_TILE


class CorrCompactInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("reads", "result_reads", "result_bases", "trimmed_reads", "trimmed_bases", "deleted_reads",
                                          "one_base", "tree", "node_limit_hits", "by_classify", "by_correct", "by_overflow")] + \
               [("ms_scan", C.c_double), ("ms_gather", C.c_double)]


CORR_ANNOT_MAX = 120  # DBGK_CORR_ANNOT_MAX


class CorrAnnotInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("suffix_bytes", C.c_uint64), ("ms_scan", C.c_double), ("ms_write", C.c_double)]


class MapParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("seed_kmers", C.c_int32), ("min_read_len", C.c_int32), ("second_alignment", C.c_int32),
                ("min_identity", C.c_double)]


MAP_HIT_DTYPE = np.dtype([("contig", "<i4"), ("read_start", "<i4"), ("read_end", "<i4"), ("contig_start", "<i4"),
                          ("contig_end", "<i4"), ("mismatches", "<i4"), ("align_len", "<i4"), ("direct", "<i4")])  # dbgk_map_hit


class MapStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("by_lds", C.c_uint64), ("by_long", C.c_uint64), ("skipped", C.c_uint64),
                ("windows_probed", C.c_uint64), ("ms_map", C.c_double), ("ms_long", C.c_double)]


ADAPTER_HIT_DTYPE = np.dtype([("adapter", "<i4"), ("score", "<i4"), ("read_start", "<i4"), ("read_end", "<i4"),
                              ("adapter_start", "<i4"), ("adapter_end", "<i4")])  # dbgk_adapter_hit

LOWQUAL_BLOCK_DTYPE = np.dtype([("error_sum", "<f8"), ("start", "<i4"), ("length", "<i4"), ("trimmed", "<i4"),
                                ("reserved", "<i4")])  # dbgk_lowqual_block


class CleanStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("by_lds", C.c_uint64), ("by_global", C.c_uint64), ("hits", C.c_uint64),
                ("cells", C.c_uint64), ("ms_lds", C.c_double), ("ms_global", C.c_double), ("ms_lowqual", C.c_double)]


CLEAN_COMPACT_TILE = 4096  # DBGK_CLEAN_COMPACT_TILE
CLEAN_KIND_LOWQUAL, CLEAN_KIND_ADAPTER = 0, 1  # DBGK_CLEAN_KIND_*


class CleanCompactInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("reads", "raw_bases", "trimmed_reads", "trimmed_bases", "short_reads", "short_bases",
                                          "clean_reads", "clean_bases")] + [("ms_scan", C.c_double), ("ms_gather", C.c_double)]


PAIR_PAIRED, PAIR_SINGLE = 0, 1  # DBGK_PAIR_*


class PairInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_pairs_in", "pair_reads", "pair_bases", "single_reads", "single_bases", "max_len")] + \
               [("ms_rank", C.c_double), ("ms_gather", C.c_double)]


PARSE_TEXT_TILE = 4096  # DBGK_PARSE_TEXT_TILE
PARSE_REC_DTYPE = np.dtype([(f, "<u4") for f in ("head_pos", "head_len", "seq_pos", "seq_len", "qual_pos", "qual_len")])  # dbgk_parse_rec


class ParseInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_records", "n_lines", "ignored_lines", "consumed", "n_bases", "max_len", "mismatched")] + \
               [(f, C.c_double) for f in ("ms_lines", "ms_states", "ms_scan", "ms_gather")]


FMT_TILE = 4096  # DBGK_FMT_TILE


class FmtInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_records", "out_bytes", "head_bytes", "suffix_bytes", "seq_bytes")] + \
               [("ms_scan", C.c_double), ("ms_gather", C.c_double)]


MAPROW_READS, MAPROW_PAIR = 1, 2  # DBGK_MAPROW_*
MAPROW_STREAMS = 3                # DBGK_MAPROW_STREAMS
MAPROW_TILE = 4096                # DBGK_MAPROW_TILE


class MapRowSide(C.Structure):    # dbgk_maprow_side
    _fields_ = [("text", C.c_void_p), ("n_text", C.c_uint64), ("recs", C.c_void_p), ("bases", C.c_void_p), ("offsets", C.c_void_p),
                ("hits", C.c_void_p)]


class MapRowInfo(C.Structure):    # dbgk_maprow_info
    _fields_ = [("n", C.c_uint64), ("counters", C.c_uint64 * 5), ("stream_bytes", C.c_uint64 * MAPROW_STREAMS), ("unprintable", C.c_uint64),
                ("ms_scan", C.c_double), ("ms_write", C.c_double)]


GZ_PIECE = 65280   # DBGK_GZ_PIECE
GZ_MAX_LEVEL = 2   # DBGK_GZ_MAX_LEVEL


class GzInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_members", "out_bytes", "stored_members", "n_literals", "n_matches", "match_bytes")]


class GzTiming(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("ms_members", "ms_match", "ms_crc_hist", "ms_codes", "ms_encode", "ms_compact")]


INF_ROUND = 4000   # DBGK_INF_ROUND
INF_REASONS = ("OK", "BLOCK_TYPE", "STORED_LEN", "STORED_PAST", "TOO_MANY_SYMS", "CL_OVER", "CL_INCOMPLETE", "CODE_OVER", "CODE_INCOMPLETE",
               "REPEAT_FIRST", "REPEAT_PAST", "NO_EOB", "BAD_LENGTH", "BAD_DISTANCE", "DISTANCE_FAR", "TRUNCATED", "GARBAGE", "OUT_MORE", "OUT_LESS",
               "CRC", "FRAME")   # DBGK_INF_*: a member's verdict is the index


class InfInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_members", "n_markers", "consumed", "out_bytes", "n_stored", "n_fixed", "n_dynamic", "n_literals", "n_matches",
                                          "n_bad", "first_bad")] + [("first_bad_reason", C.c_uint32)]


class InfTiming(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("ms_decode", "ms_resolve", "ms_scan")]


class LinkParams(C.Structure):
    _fields_ = [("mate_pair", C.c_int32), ("pair_num_cut", C.c_int32), ("insert_size", C.c_int32)]


LINK_PAIR_DTYPE = np.dtype([("contig1", "<i4"), ("start1", "<i4"), ("end1", "<i4"), ("contig2", "<i4"), ("start2", "<i4"),
                            ("end2", "<i4"), ("direct1", "u1"), ("direct2", "u1"), ("pad", "u1", (2,)), ("reserved", "<i4")])  # dbgk_link_pair
LINK_ENTRY_DTYPE = np.dtype([("target", "<u4"), ("freq", "<u4"), ("size", "<i8")])  # dbgk_link_entry
LINK_ITEM_DTYPE = np.dtype([("contig", "<i4"), ("value", "<i4")])  # dbgk_link_item


class LinkCounters(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("fr", "rf", "ff", "rr", "wrong")]


class LinkSummary(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("lowfreq", "interleave", "repeat_nodes", "deleted", "scaffolds", "items")]


class LinkTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("records", "kept", "entries", "links", "emit_bytes")] + \
               [(f, C.c_double) for f in ("ms_orient", "ms_sort", "ms_reduce", "ms_chain", "ms_emit")]


class FillParams(C.Structure):
    _fields_ = [("pair_num_cut", C.c_int32), ("reserved", C.c_int32 * 3)]


FILL_RECORD_DTYPE = np.dtype([("read", "<i4"), ("read_len", "<i4"), ("align1_end", "<i4"), ("align2_start", "<i4"), ("contig1", "<i4"),
                              ("contig2", "<i4"), ("direct1", "u1"), ("direct2", "u1"), ("pad", "u1", (2,)), ("reserved", "<i4")])  # dbgk_fill_record
FILL_GAPSTAT_DTYPE = np.dtype([("contig_lo", "<i4"), ("contig_hi", "<i4"), ("mode", "<i4"), ("mode_freq", "<i4"), ("total_freq", "<i4"),
                               ("variance", "<i4")])  # dbgk_fill_gapstat
FILL_ITEM_DTYPE = np.dtype([("contig", "<i4"), ("reversed", "<i4"), ("length", "<u4"), ("gap", "<i4"), ("cons_off", "<u8")])  # dbgk_fill_item
FILL_GAP_DTYPE = np.dtype([("mode", "<i4"), ("mode_freq", "<i4"), ("total_freq", "<i4"), ("variance", "<i4"), ("identity", "<f4"),
                           ("host_path", "<i4")])  # dbgk_fill_gap


class FillSummary(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("lowfreq", "repeat_nodes", "deleted", "scaffolds", "items", "gaps", "filled", "cons_bytes", "pairs")]


class FillTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("records", "pooled", "links", "cons_bytes", "span_bytes", "emit_bytes")] + \
               [(f, C.c_double) for f in ("ms_orient", "ms_sort", "ms_table", "ms_gapstat", "ms_consensus", "ms_emit")]


class SuperParams(C.Structure):
    _fields_ = [("pair_num_cut", C.c_int32), ("reserved", C.c_int32 * 3)]


SUPER_GAPSTAT_DTYPE = np.dtype([("contig_lo", "<i4"), ("contig_hi", "<i4"), ("mean", "<i4"), ("min", "<i4"), ("max", "<i4"), ("total", "<i4"),
                                ("variance", "<i4"), ("reserved", "<i4")])  # dbgk_super_gapstat
SUPER_JUNCTION_DTYPE = np.dtype([("left_contig", "<i4"), ("right_contig", "<i4"), ("mean", "<i4"), ("min", "<i4"), ("max", "<i4"),
                                 ("total", "<i4"), ("variance", "<i4"), ("n_written", "<i4"), ("gap_id", "<i4"), ("median", "<i4"),
                                 ("first_slice", "<u8"), ("n_slices", "<u4"), ("n_kept", "<u4")])  # dbgk_super_junction
SUPER_SLICE_DTYPE = np.dtype([("record", "<u8"), ("offset", "<u8"), ("length", "<u4"), ("reversed", "u1"), ("kept", "u1"),
                              ("pad", "u1", (2,))])  # dbgk_super_slice


class SuperSummary(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("lowfreq", "interleave", "repeat_nodes", "deleted", "scaffolds", "items", "junctions", "slices",
                                          "lines", "slice_bytes", "pairs")] + \
               [("bad_record", C.c_int64), ("bad_read", C.c_int64), ("bad_left", C.c_int32), ("bad_right", C.c_int32)]


class SuperTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("records", "pooled", "links", "slice_bytes", "emit_bytes")] + \
               [(f, C.c_double) for f in ("ms_orient", "ms_sort", "ms_table", "ms_gapstat", "ms_slices", "ms_emit")]


class ContigParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("kmer_freq_cutoff", C.c_int32), ("contig_len_cutoff", C.c_int32), ("reserved", C.c_int32)]


CONTIG_RECORD_DTYPE = np.dtype([("anchor", "<u8"), ("left_end", "<u8"), ("right_end", "<u8"), ("left_len", "<u4"), ("right_len", "<u4"),
                                ("left_depth", "<u4"), ("right_depth", "<u4"), ("left_mark", "u1"), ("right_mark", "u1"),
                                ("left_repeat", "u1"), ("right_repeat", "u1"), ("host_walked", "u1"), ("mid_depth", "u1"),
                                ("pad", "u1", (2,))])  # dbgk_contig_record


class ContigSummary(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("contigs", "kernel_contigs", "host_contigs", "bytes", "linear_nodes", "host_nodes", "rounds",
                                          "reserved")]


class ContigTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("upload_bytes", "emit_bytes")] + \
               [(f, C.c_double) for f in ("ms_upload", "ms_compact", "ms_successors", "ms_mutual", "ms_rank", "ms_place", "ms_scatter",
                                          "ms_emit", "ms_host_walk")]


TRACE_REQUEST_DTYPE = np.dtype([("slot", "<u8"), ("direct", "<i4"), ("reserved", "<i4")])  # dbgk_trace_request
TRACE_ROW_DTYPE = np.dtype([("start", "<u4"), ("last", "<u4"), ("len", "<u4"), ("depth", "<u4"), ("direct", "i1"), ("mark", "u1"),
                            ("status", "u1"), ("pad", "u1"), ("reserved", "<u4")])  # dbgk_trace_row
TRACE_TRACED, TRACE_BELOW_CUTOFF, TRACE_ABSENT, TRACE_NOT_LINEAR = 0, 1, 2, 3
TRACE_MAX_CUTOFF = 65536


class TraceSummary(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("rows", "traced", "nodes", "batches")]


ALIGN_ROW_DTYPE = np.dtype([("len_i", "<u4"), ("len_j", "<u4"), ("score", "<i4"), ("aligned_len", "<u4"), ("diffs", "<u4"), ("status", "u1"),
                            ("pad", "u1", (3,))])  # dbgk_align_row
ALIGN_MAX_LEN = 256
ALIGN_DONE, ALIGN_TOO_LONG = 0, 1


class AlignSummary(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("pairs", "aligned", "too_long", "batches", "aligned_bytes", "reserved")]


class AlignTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("bytes_up", "bytes_back", "batches", "pairs", "cells", "reserved")] + [("ms_align", C.c_double)]


class SimplifyTiming(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("bytes_returned", "batches", "updated_slots", "reserved")] + \
               [(f, C.c_double) for f in ("ms_trace", "ms_branches", "ms_fill", "ms_update")]


class DbgkError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        L = lib()
        msg = "%s: %s" % (what, L.dbgk_strerror(status).decode())
        if status == ERR_HIP:
            msg += " [%s]" % L.dbgk_last_error().decode()
        super().__init__(msg)


# every symbol include/dbgk.h declares: (name, restype, argtypes)
_u64, _vp, _i = C.c_uint64, C.c_void_p, C.c_int
SYMBOLS = [
    ("dbgk_create", _i, [C.POINTER(Config), C.POINTER(_vp)]),
    ("dbgk_destroy", _i, [_vp]),
    ("dbgk_reset", _i, [_vp]),
    ("dbgk_push_reads", _i, [_vp, _vp, _vp, _u64]),
    ("dbgk_push_acquire", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u64)]),
    ("dbgk_push_commit", _i, [_vp, _u64]),
    ("dbgk_push_reads_device", _i, [_vp, _vp, _vp, _u64, _u64]),
    ("dbgk_pack_bases", _i, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_pack_reads", _i, [_vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_unpack_bases", _i, [_vp, _u64, _u64, _vp]),
    ("dbgk_push_reads_packed", _i, [_vp, _vp, _vp, _u64, _u64]),
    ("dbgk_push_commit_packed", _i, [_vp, _u64, _u64]),
    ("dbgk_push_reads_packed_device", _i, [_vp, _vp, _vp, _u64, _u64]),
    ("dbgk_pack_bases_device", _i, [_vp, _vp, _u64, _vp]),
    ("dbgk_push_reads_packed_uniform", _i, [_vp, _vp, _u64, C.c_uint32, _u64]),
    ("dbgk_push_reads_packed_uniform_device", _i, [_vp, _vp, _u64, C.c_uint32]),
    ("dbgk_finalize", _i, [_vp, C.POINTER(Stats)]),
    ("dbgk_sync", _i, [_vp]),
    ("dbgk_resize_table", _i, [_vp, _u64]),
    ("dbgk_flush", _i, [_vp]),
    ("dbgk_store_room", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    ("dbgk_copy_nodes_peer", _i, [_vp, _vp, _vp, _vp, _u64]),
    ("dbgk_export_host_table", _i, [_vp, _u64, _vp, _vp]),
    ("dbgk_export_host_table_links", _i, [_vp, _u64, _vp, _vp, C.c_int32, _vp, _vp, _vp, _u64, C.POINTER(_u64), _vp, _u64, C.POINTER(_u64), _vp]),
    ("dbgk_export_sorted", _i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_export_first_seen_order", _i, [_vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_digest", _i, [_vp, C.POINTER(_u64)]),
    ("dbgk_link_stats_device", _i, [_vp, C.c_int32, C.POINTER(LinkStats)]),
    ("dbgk_wide_export_sorted", _i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_wide_export_host_table", _i, [_vp, _u64, _vp, _vp]),
    ("dbgk_wide_export_host_table_links", _i, [_vp, _u64, _vp, _vp, C.c_int32, _vp, _vp, _vp, _u64, C.POINTER(_u64), _vp, _u64, C.POINTER(_u64), _vp]),
    ("dbgk_wide_partition_export", _i, [_vp, C.c_uint32, _vp, _u64, _vp]),
    ("dbgk_wide_merge_nodes", _i, [_vp, _vp, _u64]),
    ("dbgk_wide_pass_info", _i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("dbgk_wide_begin_pass", _i, [_vp, C.c_uint32]),
    ("dbgk_wide_end_pass", _i, [_vp]),
    ("dbgk_shard_side_export", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_shard_side_clear", _i, [_vp]),
    ("dbgk_seed_export_sorted", _i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_seed_export_host_table", _i, [_vp, _u64, _vp, _vp]),
    ("dbgk_kfreq_export_counts", _i, [_vp, _u64, _u64, _vp]),
    ("dbgk_kfreq_export_bits", _i, [_vp, C.c_uint32, _u64, _u64, _vp]),
    ("dbgk_kfreq_merge_counts", _i, [_vp, _vp, _u64, _u64]),
    ("dbgk_kfreq_device_counts", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_kfreq_spectrum", _i, [_vp, _u64, _u64, _vp]),
    ("dbgk_kfreq_spectrum_ms", _i, [_vp, C.POINTER(C.c_double)]),
    ("dbgk_extract_kmers", _i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    ("dbgk_partition_counts", _i, [_vp, C.c_uint32, _vp]),
    ("dbgk_partition_export", _i, [_vp, C.c_uint32, _vp, _u64]),
    ("dbgk_merge_nodes", _i, [_vp, _vp, _u64]),
    ("dbgk_refresh_stats", _i, [_vp, C.POINTER(Stats)]),
    ("dbgk_plan_partition", _i, [_u64, _u64, C.c_uint32, C.c_uint32, C.POINTER(PlanInfo)]),
    ("dbgk_shard_buffers", _i, [_vp, C.POINTER(ShardInfo)]),
    ("dbgk_shard_mark_exchanged", _i, [_vp]),
    ("dbgk_shard_plan", _i, [_vp]),
    ("dbgk_shard_build_range", _i, [_vp, C.c_uint32, C.c_uint32]),
    ("dbgk_shard_outgoing", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_shard_overflow", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_shard_heavy", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_shard_merge", _i, [_vp, _vp, _u64, _i, _i]),
    ("dbgk_add_polyA", _i, [_vp, C.c_uint32, C.c_uint32]),
    ("dbgk_memcpy_d2d", _i, [_vp, _vp, _vp, C.c_size_t]),
    ("dbgk_comm_create", _i, [C.POINTER(Config), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(_vp)]),
    ("dbgk_comm_destroy", _i, [_vp]),
    ("dbgk_comm_size", C.c_uint32, [_vp]),
    ("dbgk_comm_handle", _vp, [_vp, C.c_uint32]),
    ("dbgk_comm_push_reads", _i, [_vp, _vp, _vp, _u64]),
    ("dbgk_comm_push_reads_packed", _i, [_vp, _vp, _vp, _u64, _u64]),
    ("dbgk_comm_flush", _i, [_vp]),
    ("dbgk_comm_refresh_stats", _i, [_vp, C.POINTER(Stats)]),
    ("dbgk_comm_finalize", _i, [_vp, C.POINTER(Stats)]),
    ("dbgk_comm_digest", _i, [_vp, C.POINTER(_u64)]),
    ("dbgk_comm_link_stats", _i, [_vp, C.c_int32, C.POINTER(LinkStats)]),
    ("dbgk_comm_export_host_table", _i, [_vp, _u64, _vp, _vp]),
    ("dbgk_comm_resize", _i, [_vp, _u64]),
    ("dbgk_comm_export_host_table_links", _i, [_vp, _u64, _vp, _vp, C.c_int32, _vp, _vp, _vp, _u64, C.POINTER(_u64), _vp, _u64, C.POINTER(_u64), _vp]),
    ("dbgk_comm_wide_export_sorted", _i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_comm_wide_export_host_table", _i, [_vp, _u64, _vp, _vp]),
    ("dbgk_comm_wide_export_host_table_links", _i, [_vp, _u64, _vp, _vp, C.c_int32, _vp, _vp, _vp, _u64, C.POINTER(_u64), _vp, _u64, C.POINTER(_u64), _vp]),
    ("dbgk_comm_kfreq_export_counts", _i, [_vp, _u64, _u64, _vp]),
    ("dbgk_comm_kfreq_export_bits", _i, [_vp, C.c_uint32, _u64, _u64, _vp]),
    ("dbgk_comm_kfreq_spectrum", _i, [_vp, _vp]),
    ("dbgk_synth_reads_device", _i, [_vp, C.POINTER(SynthParams), _u64, _u64, _vp, _vp]),
    ("dbgk_device_malloc", _i, [_vp, C.c_size_t, C.POINTER(_vp)]),
    ("dbgk_device_free", _i, [_vp, _vp]),
    ("dbgk_memcpy_d2h", _i, [_vp, _vp, _vp, C.c_size_t]),
    ("dbgk_memcpy_h2d", _i, [_vp, _vp, _vp, C.c_size_t]),
    ("dbgk_get_timings", _i, [_vp, C.POINTER(Timings)]),
    ("dbgk_reset_timings", _i, [_vp]),
    ("dbgk_stream", _vp, [_vp]),
    ("dbgk_measure_copy_bandwidth", _i, [_vp, C.c_size_t, _i, C.POINTER(C.c_double)]),
    ("dbgk_measure_copy_bandwidth2", _i, [_vp, C.c_size_t, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("dbgk_measure_gather_bandwidth", _i, [_vp, C.c_size_t, _u64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("dbgk_corr_create", _i, [C.POINTER(CorrParams), _i, C.POINTER(_vp)]),
    ("dbgk_corr_destroy", _i, [_vp]),
    ("dbgk_corr_load_bits", _i, [_vp, _u64, _u64, _vp]),
    ("dbgk_corr_seal", _i, [_vp]),
    ("dbgk_corr_from_kfreq", _i, [_vp, _vp, C.c_uint32]),
    ("dbgk_corr_table_stats", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    ("dbgk_corr_export_bits", _i, [_vp, _u64, _u64, _vp]),
    ("dbgk_corr_reads", _i, [_vp, _vp, _vp, _u64, _vp, _vp]),
    ("dbgk_corr_batch_stats", _i, [_vp, C.POINTER(CorrStats)]),
    ("dbgk_corr_mutation_scan", _i, [_vp, _vp, _vp, _u64, C.c_uint32, _vp]),
    ("dbgk_corr_mutation_scan_ms", _i, [_vp, C.POINTER(C.c_double)]),
    ("dbgk_corr_reads_device", _i, [_vp, _vp, _vp, _u64, _vp]),
    ("dbgk_corr_compact", _i, [_vp, C.POINTER(CorrCompactInfo)]),
    ("dbgk_corr_compact_from", _i, [_vp, _vp, _vp, _vp, _u64, C.POINTER(CorrCompactInfo)]),
    ("dbgk_corr_compact_results", _i, [_vp, _vp, _vp]),
    ("dbgk_corr_compact_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u64)]),
    ("dbgk_corr_annot", _i, [_vp, C.POINTER(CorrAnnotInfo)]),
    ("dbgk_corr_annot_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u64)]),
    ("dbgk_corr_annot_results", _i, [_vp, _vp, _vp]),
    ("dbgk_push_corrected", _i, [_vp, _vp]),
    ("dbgk_map_create", _i, [C.POINTER(MapParams), _i, C.POINTER(_vp)]),
    ("dbgk_map_destroy", _i, [_vp]),
    ("dbgk_map_set_contigs", _i, [_vp, _vp, _vp, _u64]),
    ("dbgk_map_set_ramp", _i, [_vp, C.c_uint32]),
    ("dbgk_map_reads", _i, [_vp, _vp, _vp, _u64, _vp]),
    ("dbgk_map_batch_stats", _i, [_vp, C.POINTER(MapStats)]),
    ("dbgk_map_reads_device", _i, [_vp, _vp, _vp, _u64, _u64, _u64, _vp]),
    ("dbgk_map_reads_device_keep", _i, [_vp, _vp, _vp, _u64, _u64, _u64]),
    ("dbgk_map_hits_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_clean_create", _i, [_i, C.POINTER(_vp)]),
    ("dbgk_clean_destroy", _i, [_vp]),
    ("dbgk_clean_set_adapters", _i, [_vp, _vp, _vp, _u64, C.c_int32]),
    ("dbgk_clean_adapter", _i, [_vp, _vp, _vp, _u64, _vp]),
    ("dbgk_clean_lowqual", _i, [_vp, _vp, _vp, _vp, _u64, C.c_double, C.c_int32, _vp]),
    ("dbgk_clean_batch_stats", _i, [_vp, C.POINTER(CleanStats)]),
    ("dbgk_clean_lowqual_device", _i, [_vp, _vp, _vp, _vp, _u64, C.c_double, C.c_int32, _vp]),
    ("dbgk_clean_adapter_device", _i, [_vp, _vp, _vp, _vp, _u64, _vp]),
    ("dbgk_clean_compact", _i, [_vp, C.c_int32, C.POINTER(CleanCompactInfo)]),
    ("dbgk_clean_compact_from", _i, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _u64, C.c_int32, C.c_int32, C.POINTER(CleanCompactInfo)]),
    ("dbgk_clean_compact_results", _i, [_vp, _vp, _vp, _vp]),
    ("dbgk_clean_compact_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u64)]),
    ("dbgk_push_cleaned", _i, [_vp, _vp]),
    ("dbgk_pair_create", _i, [_i, C.POINTER(_vp)]),
    ("dbgk_pair_destroy", _i, [_vp]),
    ("dbgk_pair_split_from", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(PairInfo)]),
    ("dbgk_pair_split_device", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(PairInfo)]),
    ("dbgk_pair_results", _i, [_vp, _i, _vp, _vp, _vp, _vp]),
    ("dbgk_pair_device", _i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u64)]),
    ("dbgk_push_pairs", _i, [_vp, _vp, _i]),
    ("dbgk_parse_create", _i, [C.c_int32, C.c_int32, _i, C.POINTER(_vp)]),
    ("dbgk_parse_destroy", _i, [_vp]),
    ("dbgk_parse_chunk", _i, [_vp, _vp, _u64, C.c_int32, C.POINTER(ParseInfo)]),
    ("dbgk_parse_chunk_device", _i, [_vp, _vp, _u64, C.c_int32, C.POINTER(ParseInfo)]),
    ("dbgk_parse_results", _i, [_vp, _vp, _vp, _vp, _vp]),
    ("dbgk_parse_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u64)]),
    ("dbgk_push_parsed", _i, [_vp, _vp]),
    ("dbgk_fmt_create", _i, [C.c_int32, C.c_int32, _i, C.POINTER(_vp)]),
    ("dbgk_fmt_destroy", _i, [_vp]),
    ("dbgk_fmt_records_device", _i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, C.POINTER(FmtInfo)]),
    ("dbgk_fmt_records_device_suffix", _i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, C.POINTER(FmtInfo)]),
    ("dbgk_fmt_records", _i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, C.POINTER(FmtInfo)]),
    ("dbgk_fmt_results", _i, [_vp, _vp, _u64]),
    ("dbgk_fmt_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_parse_recs_device", _i, [_vp, C.POINTER(_vp)]),
    ("dbgk_parse_text_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_maprow_create", _i, [C.c_int32, C.c_char_p, C.c_int32, _i, C.POINTER(_vp)]),
    ("dbgk_maprow_destroy", _i, [_vp]),
    ("dbgk_maprow_set_contigs", _i, [_vp, _vp, _vp, _vp, _u64]),
    ("dbgk_maprow_take_hits", _i, [_vp, C.c_int32, _vp]),
    ("dbgk_maprow_rows_device", _i, [_vp, C.POINTER(MapRowSide), _u64, C.POINTER(MapRowInfo)]),
    ("dbgk_maprow_rows", _i, [_vp, C.POINTER(MapRowSide), _u64, C.POINTER(MapRowInfo)]),
    ("dbgk_maprow_device", _i, [_vp, C.c_int32, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_maprow_results", _i, [_vp, C.c_int32, _vp, _u64]),
    ("dbgk_gz_create", _i, [_i, C.POINTER(_vp)]),
    ("dbgk_gz_destroy", _i, [_vp]),
    ("dbgk_gz_deflate", _i, [_vp, _vp, _u64, _i, C.POINTER(GzInfo)]),
    ("dbgk_gz_deflate_device", _i, [_vp, _vp, _u64, _i, C.POINTER(GzInfo)]),
    ("dbgk_gz_results", _i, [_vp, _vp, _u64]),
    ("dbgk_gz_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_gz_timing_get", _i, [_vp, C.POINTER(GzTiming)]),
    ("dbgk_inf_create", _i, [_u64, C.POINTER(_vp)]),
    ("dbgk_inf_destroy", _i, [_vp]),
    ("dbgk_inf_inflate", _i, [_vp, _vp, _u64, _i, C.POINTER(InfInfo)]),
    ("dbgk_inf_inflate_device", _i, [_vp, _vp, _u64, C.POINTER(_u64), _u64, C.POINTER(InfInfo)]),
    ("dbgk_inf_results", _i, [_vp, _vp, _u64]),
    ("dbgk_inf_device", _i, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    ("dbgk_inf_member_status", _i, [_vp, _vp, _u64]),
    ("dbgk_inf_timing_get", _i, [_vp, C.POINTER(InfTiming)]),
    ("dbgk_link_create", _i, [C.POINTER(LinkParams), _i, C.POINTER(_vp)]),
    ("dbgk_link_destroy", _i, [_vp]),
    ("dbgk_link_set_contigs", _i, [_vp, _vp, _u64]),
    ("dbgk_link_add_pairs", _i, [_vp, _vp, _u64]),
    ("dbgk_link_add_hits", _i, [_vp, _vp, _vp, _u64]),
    ("dbgk_link_build", _i, [_vp]),
    ("dbgk_link_export", _i, [_vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(LinkCounters)]),
    ("dbgk_link_resolve", _i, [_vp, C.POINTER(LinkSummary)]),
    ("dbgk_link_snapshot", _i, [_vp, C.c_int32, _vp, _vp, _vp]),
    ("dbgk_link_layout", _i, [_vp, _vp, _vp, _vp]),
    ("dbgk_link_emit", _i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_link_batch_stats", _i, [_vp, C.POINTER(LinkTiming)]),
    ("dbgk_fill_create", _i, [C.POINTER(FillParams), _i, C.POINTER(_vp)]),
    ("dbgk_fill_destroy", _i, [_vp]),
    ("dbgk_fill_set_contigs", _i, [_vp, _vp, _u64]),
    ("dbgk_fill_set_reads", _i, [_vp, _vp, _vp, _u64]),
    ("dbgk_fill_add_records", _i, [_vp, _vp, _u64]),
    ("dbgk_fill_add_hits", _i, [_vp, _vp, _u64, _u64]),
    ("dbgk_fill_build", _i, [_vp]),
    ("dbgk_fill_export", _i, [_vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(LinkCounters)]),
    ("dbgk_fill_gap_stats", _i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_fill_resolve", _i, [_vp, C.POINTER(FillSummary)]),
    ("dbgk_fill_snapshot", _i, [_vp, C.c_int32, _vp, _vp, _vp]),
    ("dbgk_fill_layout", _i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    ("dbgk_fill_emit", _i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_fill_batch_stats", _i, [_vp, C.POINTER(FillTiming)]),
    ("dbgk_super_create", _i, [C.POINTER(SuperParams), _i, C.POINTER(_vp)]),
    ("dbgk_super_destroy", _i, [_vp]),
    ("dbgk_super_set_contigs", _i, [_vp, _vp, _u64]),
    ("dbgk_super_set_reads", _i, [_vp, _vp, _vp, _u64]),
    ("dbgk_super_add_records", _i, [_vp, _vp, _u64]),
    ("dbgk_super_add_hits", _i, [_vp, _vp, _u64, _u64]),
    ("dbgk_super_build", _i, [_vp]),
    ("dbgk_super_export", _i, [_vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(LinkCounters)]),
    ("dbgk_super_gap_stats", _i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_super_resolve", _i, [_vp, C.POINTER(SuperSummary)]),
    ("dbgk_super_snapshot", _i, [_vp, C.c_int32, _vp, _vp, _vp]),
    ("dbgk_super_layout", _i, [_vp, _vp, _vp, _vp, _vp]),
    ("dbgk_super_slices", _i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_super_slice_bytes", _i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_super_emit", _i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    ("dbgk_super_batch_stats", _i, [_vp, C.POINTER(SuperTiming)]),
    ("dbgk_contig_create", _i, [C.POINTER(ContigParams), _i, C.POINTER(_vp)]),
    ("dbgk_contig_destroy", _i, [_vp]),
    ("dbgk_contig_set_table", _i, [_vp, _u64, _vp, _vp, _vp, _vp]),
    ("dbgk_contig_read_out", _i, [_vp, C.POINTER(ContigSummary)]),
    ("dbgk_contig_summary_get", _i, [_vp, C.POINTER(ContigSummary)]),
    ("dbgk_contig_results", _i, [_vp, _vp, _vp, _vp, _vp]),
    ("dbgk_contig_timing_get", _i, [_vp, C.POINTER(ContigTiming)]),
    ("dbgk_wide_contig_create", _i, [C.POINTER(ContigParams), _i, C.POINTER(_vp)]),
    ("dbgk_wide_contig_set_table", _i, [_vp, _u64, _vp, _vp, _vp, _vp]),
    ("dbgk_simplify_trace", _i, [_vp, _vp, _u64, C.c_int32, C.POINTER(TraceSummary)]),
    ("dbgk_simplify_trace_branches", _i, [_vp, _vp, _u64, C.c_int32, C.POINTER(TraceSummary)]),
    ("dbgk_simplify_trace_results", _i, [_vp, _vp, _vp, _vp, _vp]),
    ("dbgk_simplify_update", _i, [_vp, _vp, _u64]),
    ("dbgk_simplify_timing_get", _i, [_vp, C.POINTER(SimplifyTiming)]),
    ("dbgk_align_pairs", _i, [_vp, _vp, _vp, _u64, C.POINTER(AlignSummary)]),
    ("dbgk_align_results", _i, [_vp, _vp, _vp, _vp, _vp]),
    ("dbgk_align_timing_get", _i, [_vp, C.POINTER(AlignTiming)]),
    ("dbgk_l1_forms_text", _i, [_vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    ("dbgk_device_count", _i, []),
    ("dbgk_abi_version", _i, []),
    ("dbgk_strerror", C.c_char_p, [_i]),
    ("dbgk_last_error", C.c_char_p, []),
]

_lib = None


def lib():
    """Load libdbgk.so (raises if it has not been built: no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C dbg_assembly_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _chk(status, what):
    if status != OK:
        raise DbgkError(status, what)


def pack_bases(bases, out=None, first_base=0):
    """ASCII bases -> 2-bit words (dbgk_pack_bases, host): -> (uint32 words, number of bytes outside ACGTNacgtn).  With `out`
    the bases are packed into that buffer from base position first_base on (boundary words are OR-ed into)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    if out is None:
        out = np.zeros((first_base + len(bases) + 15) // 16, dtype=np.uint32)
    other = C.c_uint64(0)
    _chk(lib().dbgk_pack_bases(bases.ctypes.data, len(bases), out.ctypes.data, first_base, C.byref(other)), "dbgk_pack_bases")
    return out, other.value


class ReadRef(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("len", C.c_uint32)]


def pack_reads(reads, out, first_base=0):
    """a list of bytes objects packed back to back into `out` from base position first_base on (dbgk_pack_reads) -> other bytes"""
    refs = (ReadRef * len(reads))()
    keep = [np.frombuffer(r, dtype=np.uint8) if len(r) else np.zeros(1, np.uint8) for r in reads]
    for i, (r, k) in enumerate(zip(reads, keep)):
        refs[i].seq, refs[i].len = k.ctypes.data, len(r)
    other = C.c_uint64(0)
    _chk(lib().dbgk_pack_reads(refs, len(reads), out.ctypes.data, first_base, C.byref(other)), "dbgk_pack_reads")
    return other.value


def unpack_bases(packed, n_bases, first_base=0):
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    out = np.empty(n_bases, dtype=np.uint8)
    _chk(lib().dbgk_unpack_bases(packed.ctypes.data, first_base, n_bases, out.ctypes.data), "dbgk_unpack_bases")
    return out


class DeviceBuffer:
    """Raw device allocation owned by a Graph handle."""

    def __init__(self, graph, nbytes):
        self.graph = graph
        self.nbytes = nbytes
        p = C.c_void_p()
        _chk(lib().dbgk_device_malloc(graph._h, nbytes, C.byref(p)), "dbgk_device_malloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            lib().dbgk_device_free(self.graph._h, self.ptr)
            self.ptr = None

    def to_host(self, dtype=np.uint8, nbytes=None):
        n = self.nbytes if nbytes is None else nbytes
        out = np.empty(n, dtype=np.uint8)
        _chk(lib().dbgk_memcpy_d2h(self.graph._h, out.ctypes.data, self.ptr, n), "dbgk_memcpy_d2h")
        return out.view(dtype)

    def from_host(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _chk(lib().dbgk_memcpy_h2d(self.graph._h, self.ptr, arr.ctypes.data, arr.nbytes), "dbgk_memcpy_h2d")


class Graph:
    """One GPU-resident k-mer graph under construction (thin wrapper over a dbgk_handle)."""

    def __init__(self, k, table_slots, max_read_len=250, device=0, engine=ENGINE_AUTO, max_batch_bases=0,
                 expected_kmers=0, shard_count=0, shard_index=0, flags=0, n_passes=0):
        self._h = None
        cfg = Config(k, max_read_len, table_slots, device, engine, max_batch_bases, expected_kmers,
                     shard_count, shard_index, flags, n_passes)
        h = C.c_void_p()
        _chk(lib().dbgk_create(C.byref(cfg), C.byref(h)), "dbgk_create")
        self._h = h
        self.k = k
        self.table_slots = table_slots
        self.stats = None

    def close(self):
        if self._h:
            lib().dbgk_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- hot path
    def push_reads(self, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _chk(lib().dbgk_push_reads(self._h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1), "dbgk_push_reads")

    def push_reads_zero_copy(self, bases, offsets):
        """the batch written straight into the handle's pinned staging buffers (dbgk_push_acquire / dbgk_push_commit), in pieces
        that fit them"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, r0 = len(offsets) - 1, 0
        while r0 < n:
            pb, po, cb, cr = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
            _chk(lib().dbgk_push_acquire(self._h, C.byref(pb), C.byref(po), C.byref(cb), C.byref(cr)), "dbgk_push_acquire")
            base0 = int(offsets[r0])
            r1 = int(np.searchsorted(offsets, base0 + cb.value, side="right")) - 1
            r1 = min(max(r1, r0 + 1), r0 + cr.value, n)
            nb = int(offsets[r1]) - base0
            assert nb <= cb.value, "a read larger than the staging buffer"
            C.memmove(pb.value, bases.ctypes.data + base0, nb)
            rel = (offsets[r0:r1 + 1] - offsets[r0]).astype(np.uint64)
            C.memmove(po.value, rel.ctypes.data, rel.nbytes)
            _chk(lib().dbgk_push_commit(self._h, r1 - r0), "dbgk_push_commit")
            r0 = r1

    def push_reads_device(self, d_bases, d_offsets, n_reads, n_bases):
        _chk(lib().dbgk_push_reads_device(self._h, d_bases, d_offsets, n_reads, n_bases), "dbgk_push_reads_device")

    # ---- the same batches, 2 bits per base (include/dbgk.h "2-bit packed reads")
    def push_reads_packed(self, packed, offsets, other_bytes=0):
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _chk(lib().dbgk_push_reads_packed(self._h, packed.ctypes.data, offsets.ctypes.data, len(offsets) - 1, other_bytes), "dbgk_push_reads_packed")

    def push_reads_packed_ptr(self, packed_ptr, offsets_ptr, n_reads, other_bytes=0):
        """host pointers (e.g. a pinned torch tensor's data_ptr)"""
        _chk(lib().dbgk_push_reads_packed(self._h, packed_ptr, offsets_ptr, n_reads, other_bytes), "dbgk_push_reads_packed")

    def push_reads_packed_zero_copy(self, bases, offsets):
        """ASCII reads packed straight into the handle's pinned staging buffers (dbgk_push_acquire / dbgk_pack_bases /
        dbgk_push_commit_packed), in pieces that fit them -- what a reader thread of the host layer does"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, r0 = len(offsets) - 1, 0
        while r0 < n:
            pb, po, cb, cr = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
            _chk(lib().dbgk_push_acquire(self._h, C.byref(pb), C.byref(po), C.byref(cb), C.byref(cr)), "dbgk_push_acquire")
            base0 = int(offsets[r0])
            r1 = int(np.searchsorted(offsets, base0 + cb.value, side="right")) - 1
            r1 = min(max(r1, r0 + 1), r0 + cr.value, n)
            nb = int(offsets[r1]) - base0
            assert nb <= cb.value, "a read larger than the staging buffer"
            C.memset(pb.value, 0, ((nb + 15) // 16) * 4)
            other = C.c_uint64(0)
            _chk(lib().dbgk_pack_bases(bases.ctypes.data + base0, nb, pb.value, 0, C.byref(other)), "dbgk_pack_bases")
            rel = (offsets[r0:r1 + 1] - offsets[r0]).astype(np.uint64)
            C.memmove(po.value, rel.ctypes.data, rel.nbytes)
            _chk(lib().dbgk_push_commit_packed(self._h, r1 - r0, other.value), "dbgk_push_commit_packed")
            r0 = r1

    def push_reads_packed_uniform(self, packed, n_reads, read_len, other_bytes=0):
        """n_reads reads of read_len bases each, packed back to back (host array or host pointer): no offsets"""
        ptr = packed if isinstance(packed, int) else np.ascontiguousarray(packed, dtype=np.uint32).ctypes.data
        _chk(lib().dbgk_push_reads_packed_uniform(self._h, ptr, n_reads, read_len, other_bytes), "dbgk_push_reads_packed_uniform")

    def push_reads_packed_uniform_device(self, d_packed, n_reads, read_len):
        _chk(lib().dbgk_push_reads_packed_uniform_device(self._h, d_packed, n_reads, read_len), "dbgk_push_reads_packed_uniform_device")

    def push_reads_packed_device(self, d_packed, d_offsets, n_reads, n_bases):
        _chk(lib().dbgk_push_reads_packed_device(self._h, d_packed, d_offsets, n_reads, n_bases), "dbgk_push_reads_packed_device")

    def pack_bases_device(self, d_bases, n_bases):
        """ASCII bases in device memory -> a DeviceBuffer of 2-bit words (dbgk_pack_bases_device)"""
        buf = DeviceBuffer(self, ((n_bases + 15) // 16) * 4 + 64)
        _chk(lib().dbgk_pack_bases_device(self._h, d_bases, n_bases, buf.ptr), "dbgk_pack_bases_device")
        return buf

    def push_corrected(self, corrector):
        """the corrector's compact batch (Corrector.compact) pushed where it lies on the device (dbgk_push_corrected)"""
        _chk(lib().dbgk_push_corrected(self._h, corrector._h), "dbgk_push_corrected")

    def push_cleaned(self, cleaner):
        """the cleaner's compact bases (Cleaner.compact) pushed where they lie on the device (dbgk_push_cleaned)"""
        _chk(lib().dbgk_push_cleaned(self._h, cleaner._h), "dbgk_push_cleaned")

    def push_pairs(self, pairer, which):
        """one output of the pair split (Pairer.split*; which = PAIR_PAIRED / PAIR_SINGLE) pushed where it lies on the device
        (dbgk_push_pairs)"""
        _chk(lib().dbgk_push_pairs(self._h, pairer._h, which), "dbgk_push_pairs")

    def push_parsed(self, parser):
        """the batch of the last chunk of a Parser pushed where it lies on the device (dbgk_push_parsed)"""
        _chk(lib().dbgk_push_parsed(self._h, parser._h), "dbgk_push_parsed")

    def finalize(self):
        st = Stats()
        _chk(lib().dbgk_finalize(self._h, C.byref(st)), "dbgk_finalize")
        self.stats = st
        return st

    def sync(self):
        _chk(lib().dbgk_sync(self._h), "dbgk_sync")

    def reset(self):
        _chk(lib().dbgk_reset(self._h), "dbgk_reset")
        self.stats = None

    def flush(self):
        _chk(lib().dbgk_flush(self._h), "dbgk_flush")

    def store_room(self):
        a, b = C.c_uint64(), C.c_uint64()
        _chk(lib().dbgk_store_room(self._h, C.byref(a), C.byref(b)), "dbgk_store_room")
        return a.value, b.value

    def resize_table(self, new_slots):
        _chk(lib().dbgk_resize_table(self._h, new_slots), "dbgk_resize_table")
        self.table_slots = new_slots

    # ---- results
    def export_sorted(self):
        n = self.stats.count
        out = np.zeros(n, dtype=NODE_DTYPE)
        got = C.c_uint64()
        _chk(lib().dbgk_export_sorted(self._h, out.ctypes.data, n, C.byref(got)), "dbgk_export_sorted")
        assert got.value == n, (got.value, n)
        return out

    def export_host_table(self, host_size=None):
        size = self.table_slots if host_size is None else host_size
        array = np.zeros(size, dtype=NODE_DTYPE)
        flags = np.zeros(size // 8 + 1, dtype=np.uint8)
        _chk(lib().dbgk_export_host_table(self._h, size, array.ctypes.data, flags.ctypes.data), "dbgk_export_host_table")
        return array, flags

    def export_host_table_links(self, cutoff=2, host_size=None):
        """dbgk_export_host_table + the consumer's whole first pass (calculate_kmer_links, contig.cpp:107-181) for that table:
        -> (array, nul_flag, klink u16[size], del_flag, tip slots, branch slots, LinkStats)"""
        size = self.table_slots if host_size is None else host_size
        array = np.zeros(size, dtype=NODE_DTYPE)
        flags = np.zeros(size // 8 + 1, dtype=np.uint8)
        klink = np.zeros(size, dtype=np.uint16)
        dele = np.zeros(size // 8 + 1, dtype=np.uint8)
        cap = int(self.stats.count)
        tips, branches = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
        nt, nb = C.c_uint64(), C.c_uint64()
        st = LinkStats()
        _chk(lib().dbgk_export_host_table_links(self._h, size, array.ctypes.data, flags.ctypes.data, cutoff, klink.ctypes.data, dele.ctypes.data,
                                                tips.ctypes.data, cap, C.byref(nt), branches.ctypes.data, cap, C.byref(nb), C.byref(st)),
             "dbgk_export_host_table_links")
        return array, flags, klink, dele, tips[:nt.value], branches[:nb.value], st

    def export_first_seen_order(self):
        n = self.stats.count - 1
        nodes = np.zeros(max(n, 1), dtype=NODE_DTYPE)
        pos = np.zeros(max(n, 1), dtype=np.uint64)
        got = C.c_uint64()
        _chk(lib().dbgk_export_first_seen_order(self._h, nodes.ctypes.data, pos.ctypes.data, n, C.byref(got)),
             "dbgk_export_first_seen_order")
        return nodes[:got.value], pos[:got.value]

    def digest(self):
        d = C.c_uint64()
        _chk(lib().dbgk_digest(self._h, C.byref(d)), "dbgk_digest")
        return d.value

    def link_stats(self, cutoff=2):
        st = LinkStats()
        _chk(lib().dbgk_link_stats_device(self._h, cutoff, C.byref(st)), "dbgk_link_stats_device")
        return st

    def extract_kmers(self, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nb = int(offsets[-1])
        kmer = np.zeros(nb, np.uint64)
        left = np.zeros(nb, np.uint8)
        right = np.zeros(nb, np.uint8)
        valid = np.zeros(nb, np.uint8)
        _chk(lib().dbgk_extract_kmers(self._h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                      kmer.ctypes.data, left.ctypes.data, right.ctypes.data, valid.ctypes.data),
             "dbgk_extract_kmers")
        return kmer, left, right, valid

    # ---- multi-GPU building blocks
    def partition_counts(self, n_parts):
        counts = np.zeros(n_parts, np.uint64)
        _chk(lib().dbgk_partition_counts(self._h, n_parts, counts.ctypes.data), "dbgk_partition_counts")
        return counts

    def partition_export(self, n_parts, d_nodes, capacity):
        _chk(lib().dbgk_partition_export(self._h, n_parts, d_nodes, capacity), "dbgk_partition_export")

    def merge_nodes(self, d_nodes, n):
        _chk(lib().dbgk_merge_nodes(self._h, d_nodes, n), "dbgk_merge_nodes")

    def refresh_stats(self):
        st = Stats()
        _chk(lib().dbgk_refresh_stats(self._h, C.byref(st)), "dbgk_refresh_stats")
        self.stats = st
        return st

    # ---- WIDE engine (128-bit keys)
    def wide_export_sorted(self):
        n = int(self.stats.count)
        out = np.zeros(n, dtype=NODE32_DTYPE)
        got = C.c_uint64()
        _chk(lib().dbgk_wide_export_sorted(self._h, out.ctypes.data, n, C.byref(got)), "dbgk_wide_export_sorted")
        assert got.value == n, (got.value, n)
        return out

    def wide_export_host_table(self, size=None):
        """size: the handle's slots (a shard: the slots of its range, default the whole table)"""
        size = self.table_slots if size is None else int(size)
        array = np.zeros(size, dtype=NODE32_DTYPE)
        flags = np.zeros(size // 8 + 1, dtype=np.uint8)
        _chk(lib().dbgk_wide_export_host_table(self._h, size, array.ctypes.data, flags.ctypes.data), "dbgk_wide_export_host_table")
        return array, flags

    def wide_export_host_table_links(self, cutoff=2, size=None):
        """dbgk_wide_export_host_table + the consumer's whole first pass for that table (k_wide_kmer_links on the device table, the
        nodes placed on the host patched in): -> (array, nul_flag, klink u16[size], del_flag, tip slots, branch slots, LinkStats)"""
        size = self.table_slots if size is None else int(size)
        array = np.zeros(size, dtype=NODE32_DTYPE)
        flags = np.zeros(size // 8 + 1, dtype=np.uint8)
        klink = np.zeros(size, dtype=np.uint16)
        dele = np.zeros(size // 8 + 1, dtype=np.uint8)
        cap = int(self.stats.count)
        tips, branches = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
        nt, nb = C.c_uint64(), C.c_uint64()
        st = LinkStats()
        _chk(lib().dbgk_wide_export_host_table_links(self._h, size, array.ctypes.data, flags.ctypes.data, cutoff, klink.ctypes.data, dele.ctypes.data,
                                                     tips.ctypes.data, cap, C.byref(nt), branches.ctypes.data, cap, C.byref(nb), C.byref(st)),
             "dbgk_wide_export_host_table_links")
        return array, flags, klink, dele, tips[:nt.value], branches[:nb.value], st

    def wide_partition_export(self, n_parts, d_nodes=None, capacity=0):
        counts = np.zeros(n_parts, np.uint64)
        _chk(lib().dbgk_wide_partition_export(self._h, n_parts, d_nodes, capacity, counts.ctypes.data), "dbgk_wide_partition_export")
        return counts

    def wide_merge_nodes(self, d_nodes, n):
        _chk(lib().dbgk_wide_merge_nodes(self._h, d_nodes, n), "dbgk_wide_merge_nodes")

    # ---- SEEDIDX engine
    SEED_DTYPE = np.dtype([("kmer", "<u8"), ("payload", "<u8")])  # payload = {id:32, pos:30, freq:1, direct:1}

    def seed_export_sorted(self):
        n = int(self.stats.count)
        out = np.zeros(max(n, 1), dtype=self.SEED_DTYPE)
        got = C.c_uint64()
        _chk(lib().dbgk_seed_export_sorted(self._h, out.ctypes.data, n, C.byref(got)), "dbgk_seed_export_sorted")
        return out[:got.value]

    def seed_export_host_table(self, host_size):
        array = np.zeros(host_size, dtype=self.SEED_DTYPE)
        flags = np.zeros(host_size // 8 + 1, dtype=np.uint8)
        _chk(lib().dbgk_seed_export_host_table(self._h, host_size, array.ctypes.data, flags.ctypes.data), "dbgk_seed_export_host_table")
        return array, flags

    # ---- KFREQ engine
    def kfreq_counts(self, first=0, n=None):
        n = (4 ** self.k - first) if n is None else n
        out = np.zeros(n, np.uint8)
        _chk(lib().dbgk_kfreq_export_counts(self._h, first, n, out.ctypes.data), "dbgk_kfreq_export_counts")
        return out

    def kfreq_bits(self, cutoff, first_byte=0, n_bytes=None):
        n_bytes = (4 ** self.k // 8 - first_byte) if n_bytes is None else n_bytes
        out = np.zeros(n_bytes, np.uint8)
        _chk(lib().dbgk_kfreq_export_bits(self._h, cutoff, first_byte, n_bytes, out.ctypes.data), "dbgk_kfreq_export_bits")
        return out

    def kfreq_spectrum(self, first=0, n=None):
        """np.uint64[256]: bin c = counters of [first, first + n) equal to c (255: 255 or more), binned on the device"""
        n = (4 ** self.k - first) if n is None else n
        out = np.zeros(256, np.uint64)
        _chk(lib().dbgk_kfreq_spectrum(self._h, first, n, out.ctypes.data), "dbgk_kfreq_spectrum")
        return out

    def kfreq_spectrum_ms(self):
        """device ms of the histogram kernel of the last kfreq_spectrum"""
        ms = C.c_double()
        _chk(lib().dbgk_kfreq_spectrum_ms(self._h, C.byref(ms)), "dbgk_kfreq_spectrum_ms")
        return ms.value

    def kfreq_device_counts(self):
        """(device address, number of counters) of a finalized KFREQ handle"""
        ptr, n = C.c_void_p(), _u64()
        _chk(lib().dbgk_kfreq_device_counts(self._h, C.byref(ptr), C.byref(n)), "dbgk_kfreq_device_counts")
        return int(ptr.value), int(n.value)

    def kfreq_merge_counts(self, d_counts, first, n):
        """counts[first, first + n) += n counters in device memory of this GPU (saturating)"""
        _chk(lib().dbgk_kfreq_merge_counts(self._h, C.c_void_p(int(d_counts)), first, n), "dbgk_kfreq_merge_counts")

    # ---- sharded table (slot-range ownership)
    def shard_info(self):
        info = ShardInfo()
        _chk(lib().dbgk_shard_buffers(self._h, C.byref(info)), "dbgk_shard_buffers")
        return info

    def shard_mark_exchanged(self):
        _chk(lib().dbgk_shard_mark_exchanged(self._h), "dbgk_shard_mark_exchanged")

    def shard_plan(self):
        _chk(lib().dbgk_shard_plan(self._h), "dbgk_shard_plan")

    def shard_build_range(self, j0, j1):
        _chk(lib().dbgk_shard_build_range(self._h, j0, j1), "dbgk_shard_build_range")

    def shard_outgoing(self):
        p, n = C.c_void_p(), C.c_uint64()
        _chk(lib().dbgk_shard_outgoing(self._h, C.byref(p), C.byref(n)), "dbgk_shard_outgoing")
        return p.value, n.value

    def shard_overflow(self):
        p, n = C.c_void_p(), C.c_uint64()
        _chk(lib().dbgk_shard_overflow(self._h, C.byref(p), C.byref(n)), "dbgk_shard_overflow")
        return p.value, n.value

    def shard_heavy(self):
        p, n = C.c_void_p(), C.c_uint64()
        _chk(lib().dbgk_shard_heavy(self._h, C.byref(p), C.byref(n)), "dbgk_shard_heavy")
        return p.value, n.value

    def shard_merge(self, d_nodes, n, is_triple=False, from_previous_shard=False):
        _chk(lib().dbgk_shard_merge(self._h, d_nodes, n, int(is_triple), int(from_previous_shard)), "dbgk_shard_merge")

    # ---- WIDE through records: passes over the input, the side table of a shard
    def wide_pass_info(self):
        a, b = C.c_uint32(), C.c_uint32()
        _chk(lib().dbgk_wide_pass_info(self._h, C.byref(a), C.byref(b)), "dbgk_wide_pass_info")
        return a.value, b.value

    def wide_begin_pass(self, p):
        _chk(lib().dbgk_wide_begin_pass(self._h, p), "dbgk_wide_begin_pass")

    def wide_end_pass(self):
        _chk(lib().dbgk_wide_end_pass(self._h), "dbgk_wide_end_pass")

    def shard_side_export(self):
        p, n = C.c_void_p(), C.c_uint64()
        _chk(lib().dbgk_shard_side_export(self._h, C.byref(p), C.byref(n)), "dbgk_shard_side_export")
        return p.value, n.value

    def shard_side_clear(self):
        _chk(lib().dbgk_shard_side_clear(self._h), "dbgk_shard_side_clear")

    def add_polyA(self, l_link, r_link):
        _chk(lib().dbgk_add_polyA(self._h, l_link, r_link), "dbgk_add_polyA")

    def memcpy_d2d(self, dst, src, nbytes):
        _chk(lib().dbgk_memcpy_d2d(self._h, dst, src, nbytes), "dbgk_memcpy_d2d")

    # ---- utilities
    def malloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def synth_reads_device(self, params, first, n_reads):
        """-> (DeviceBuffer bases, DeviceBuffer offsets, n_bases)"""
        nb = n_reads * params.read_len
        d_bases = self.malloc(nb + 64)
        d_off = self.malloc((n_reads + 1) * 8)
        _chk(lib().dbgk_synth_reads_device(self._h, C.byref(params), first, n_reads, d_bases.ptr, d_off.ptr),
             "dbgk_synth_reads_device")
        return d_bases, d_off, nb

    def timings(self):
        t = Timings()
        _chk(lib().dbgk_get_timings(self._h, C.byref(t)), "dbgk_get_timings")
        return t

    def reset_timings(self):
        _chk(lib().dbgk_reset_timings(self._h), "dbgk_reset_timings")

    def l1_forms(self):
        """the level-1 kernel forms launched since the last reset / reset_timings, in launch order: a list of the forms' texts
        (dbgk_l1_forms_text; the first 16 launches -- `l1_launches` gets the number of all of them)"""
        buf, n = C.create_string_buffer(4096), C.c_uint32()
        _chk(lib().dbgk_l1_forms_text(self._h, buf, len(buf), C.byref(n)), "dbgk_l1_forms_text")
        self.l1_launches = n.value
        return buf.value.decode().splitlines()

    def copy_bandwidth(self, nbytes=1 << 30, iters=10):
        g = C.c_double()
        _chk(lib().dbgk_measure_copy_bandwidth(self._h, nbytes, iters, C.byref(g)), "dbgk_measure_copy_bandwidth")
        return g.value

    def copy_bandwidth_detail(self, nbytes=1 << 30, iters=10):
        """(best of the library's copy kernels and the runtime's memcpy, the runtime's hipMemcpyDtoD alone), GB/s read + written"""
        g, m = C.c_double(), C.c_double()
        _chk(lib().dbgk_measure_copy_bandwidth2(self._h, nbytes, iters, C.byref(g), C.byref(m)), "dbgk_measure_copy_bandwidth2")
        return g.value, m.value

    def gather_bandwidth(self, nbytes=16 << 30, n_accesses=1 << 30):
        """random 64-byte sectors of an nbytes buffer: (GB/s, G sectors/s)"""
        g, a = C.c_double(), C.c_double()
        _chk(lib().dbgk_measure_gather_bandwidth(self._h, nbytes, n_accesses, C.byref(g), C.byref(a)), "dbgk_measure_gather_bandwidth")
        return g.value, a.value


class Comm:
    """N sharded handles of one table inside this process (dbgk_comm_*): the C++ host layer's multi-GPU path."""

    def __init__(self, k, table_slots, devices, max_read_len=250, expected_kmers=0, max_batch_bases=0, engine=ENGINE_PARTITION):
        self._c = None
        cfg = Config(k, max_read_len, table_slots, 0, engine, max_batch_bases, expected_kmers, 0, 0, 0)
        dev = (C.c_int32 * len(devices))(*devices)
        c = C.c_void_p()
        _chk(lib().dbgk_comm_create(C.byref(cfg), dev, len(devices), C.byref(c)), "dbgk_comm_create")
        self._c = c
        self.k = k
        self.table_slots = table_slots
        self.stats = None

    def close(self):
        if self._c:
            lib().dbgk_comm_destroy(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def push_reads(self, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _chk(lib().dbgk_comm_push_reads(self._c, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1), "dbgk_comm_push_reads")

    def export_host_table_links(self, host_size, count, cutoff=2):
        """dbgk_comm_export_host_table_links -> (array, nul_flag, klink u16[size], del_flag, tip slots, branch slots, LinkStats)"""
        array = np.zeros(host_size, dtype=NODE_DTYPE)
        flags = np.zeros(host_size // 8 + 1, dtype=np.uint8)
        klink = np.zeros(host_size, dtype=np.uint16)
        dele = np.zeros(host_size // 8 + 1, dtype=np.uint8)
        cap = int(count)
        tips, branches = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
        nt, nb = C.c_uint64(), C.c_uint64()
        st = LinkStats()
        _chk(lib().dbgk_comm_export_host_table_links(self._c, host_size, array.ctypes.data, flags.ctypes.data, cutoff, klink.ctypes.data, dele.ctypes.data,
                                                     tips.ctypes.data, cap, C.byref(nt), branches.ctypes.data, cap, C.byref(nb), C.byref(st)),
             "dbgk_comm_export_host_table_links")
        return array, flags, klink, dele, tips[:nt.value], branches[:nb.value], st

    def push_reads_packed(self, packed, offsets, other_bytes=0):
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _chk(lib().dbgk_comm_push_reads_packed(self._c, packed.ctypes.data, offsets.ctypes.data, len(offsets) - 1, other_bytes), "dbgk_comm_push_reads_packed")

    def flush(self):
        _chk(lib().dbgk_comm_flush(self._c), "dbgk_comm_flush")

    def resize(self, new_slots):
        _chk(lib().dbgk_comm_resize(self._c, new_slots), "dbgk_comm_resize")
        self.table_slots = new_slots

    def refresh_stats(self):
        st = Stats()
        _chk(lib().dbgk_comm_refresh_stats(self._c, C.byref(st)), "dbgk_comm_refresh_stats")
        return st

    def finalize(self):
        st = Stats()
        _chk(lib().dbgk_comm_finalize(self._c, C.byref(st)), "dbgk_comm_finalize")
        self.stats = st
        return st

    def digest(self):
        d = C.c_uint64()
        _chk(lib().dbgk_comm_digest(self._c, C.byref(d)), "dbgk_comm_digest")
        return d.value

    def link_stats(self, cutoff=2):
        st = LinkStats()
        _chk(lib().dbgk_comm_link_stats(self._c, cutoff, C.byref(st)), "dbgk_comm_link_stats")
        return st

    def export_host_table(self, host_size=None):
        size = self.table_slots if host_size is None else host_size
        array = np.zeros(size, dtype=NODE_DTYPE)
        flags = np.zeros(size // 8 + 1, dtype=np.uint8)
        _chk(lib().dbgk_comm_export_host_table(self._c, size, array.ctypes.data, flags.ctypes.data), "dbgk_comm_export_host_table")
        return array, flags

    # ---- a communicator of WIDE handles (engine=ENGINE_WIDE, k <= 63)
    def wide_export_sorted(self):
        n = int(self.stats.count)
        out = np.zeros(n, dtype=NODE32_DTYPE)
        got = C.c_uint64()
        _chk(lib().dbgk_comm_wide_export_sorted(self._c, out.ctypes.data, n, C.byref(got)), "dbgk_comm_wide_export_sorted")
        return out[:got.value]

    def wide_export_host_table(self):
        size = self.table_slots
        array = np.zeros(size, dtype=NODE32_DTYPE)
        flags = np.zeros(size // 8 + 1, dtype=np.uint8)
        _chk(lib().dbgk_comm_wide_export_host_table(self._c, size, array.ctypes.data, flags.ctypes.data), "dbgk_comm_wide_export_host_table")
        return array, flags

    def wide_export_host_table_links(self, cutoff=2):
        """dbgk_comm_wide_export_host_table_links -> (array, nul_flag, klink u16[size], del_flag, tip slots, branch slots, LinkStats)"""
        size = self.table_slots
        array = np.zeros(size, dtype=NODE32_DTYPE)
        flags = np.zeros(size // 8 + 1, dtype=np.uint8)
        klink = np.zeros(size, dtype=np.uint16)
        dele = np.zeros(size // 8 + 1, dtype=np.uint8)
        cap = int(self.stats.count)
        tips, branches = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
        nt, nb = C.c_uint64(), C.c_uint64()
        st = LinkStats()
        _chk(lib().dbgk_comm_wide_export_host_table_links(self._c, size, array.ctypes.data, flags.ctypes.data, cutoff, klink.ctypes.data, dele.ctypes.data,
                                                          tips.ctypes.data, cap, C.byref(nt), branches.ctypes.data, cap, C.byref(nb), C.byref(st)),
             "dbgk_comm_wide_export_host_table_links")
        return array, flags, klink, dele, tips[:nt.value], branches[:nb.value], st

    # ---- a communicator of frequency tables (engine=ENGINE_KFREQ)
    def kfreq_counts(self, first=0, n=None):
        n = 4 ** self.k - first if n is None else n
        out = np.empty(n, dtype=np.uint8)
        _chk(lib().dbgk_comm_kfreq_export_counts(self._c, first, n, out.ctypes.data), "dbgk_comm_kfreq_export_counts")
        return out

    def kfreq_bits(self, cutoff, first_byte=0, n_bytes=None):
        n_bytes = 4 ** self.k // 8 - first_byte if n_bytes is None else n_bytes
        out = np.empty(n_bytes, dtype=np.uint8)
        _chk(lib().dbgk_comm_kfreq_export_bits(self._c, cutoff, first_byte, n_bytes, out.ctypes.data), "dbgk_comm_kfreq_export_bits")
        return out

    def kfreq_spectrum(self):
        """np.uint64[256] over the whole table: every member bins the range it owns"""
        out = np.zeros(256, np.uint64)
        _chk(lib().dbgk_comm_kfreq_spectrum(self._c, out.ctypes.data), "dbgk_comm_kfreq_spectrum")
        return out


# ---- host helpers mirrored from the reference (kmerSet.cpp:72-95), needed to size tables ---------

def is_prime_ref(num):
    """kmerSet.cpp:72-81, including its float-sqrt / strict-< quirk (9, 25, 49 ... pass)."""
    if num < 4:
        return True
    if num % 2 == 0:
        return False
    bound = int(np.sqrt(np.float32(num)))
    i = 3
    while i < bound:
        if num % i == 0:
            return False
        i += 2
    return True


def find_next_prime_ref(num):
    """kmerSet.cpp:85-95"""
    if num % 2 == 0:
        num += 1
    while not is_prime_ref(num):
        num += 2
    return num


def plan_partition(table_slots, expected_kmers, shard_count=0, shard_index=0):
    """geometry of a PARTITION handle with these parameters, computed on the host (no device is touched): PlanInfo"""
    info = PlanInfo()
    _chk(lib().dbgk_plan_partition(table_slots, expected_kmers, shard_count, shard_index, C.byref(info)), "dbgk_plan_partition")
    return info


class _Handle:
    """What the stage classes share: the handle `_h` of the C library, destroyed once by the C function `_destroy` names, and the
    context manager that closes it."""
    _destroy = None

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DeviceSuffixes(collections.namedtuple("DeviceSuffixes", "d_suffix d_offsets n n_bytes")):
    """A suffix plane in device memory: the pointer of its bytes (16-byte aligned; None with d_offsets None for all empty), the pointer of
    its n + 1 uint64 offsets, the records and the bytes.  Corrector.annotate_device returns one; Formatter.format_device reads it where
    it lies."""


class Corrector(_Handle):
    """correct_error_reads on the GPU (CORRECT section of include/dbgk.h).  Defaults are the reference's: -m and -x are
    17 whatever k is.  Build the table with load_file (a 1-bit .cz file: raw blocks, then the loader's mirror) or
    from_kfreq (a finalized KFREQ Graph + cutoff), then correct(bases, offsets)."""
    _destroy = "dbgk_corr_destroy"
    BLOCK_BYTES = 1 << 20  # one compressed block of the .cz file: 8 Mi k-mers

    def __init__(self, k=17, m=17, c=2, x=17, n=5000000, r=75, device=0):
        self.k = k
        self._h = C.c_void_p()
        _chk(lib().dbgk_corr_create(C.byref(CorrParams(k, m, c, x, n, r)), device, C.byref(self._h)), "dbgk_corr_create")

    def load_bits(self, first_byte, raw):
        raw = np.ascontiguousarray(np.frombuffer(bytes(raw), dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw, dtype=np.uint8)
        _chk(lib().dbgk_corr_load_bits(self._h, first_byte, raw.size, raw.ctypes.data), "dbgk_corr_load_bits")

    def seal(self):
        _chk(lib().dbgk_corr_seal(self._h), "dbgk_corr_seal")

    def load_file(self, path):
        """a 1-bit .cz table (+ .cz.len) as kmerfreq -b 1 writes it, loaded like make_kmerFreq_1bit_table_from_1BitGz"""
        import zlib
        lens = [int(v) for v in open(path + ".len").read().split()]
        table_bytes = max(4 ** self.k // 8, 1)
        with open(path, "rb") as f:
            for b, n in enumerate(lens):
                blk = zlib.decompress(f.read(n))
                at = b * self.BLOCK_BYTES
                if at < table_bytes:
                    self.load_bits(at, blk[:table_bytes - at])
        self.seal()

    def from_kfreq(self, graph, cutoff):
        _chk(lib().dbgk_corr_from_kfreq(self._h, graph._h, cutoff), "dbgk_corr_from_kfreq")

    def table_stats(self):
        t, h = _u64(), _u64()
        _chk(lib().dbgk_corr_table_stats(self._h, C.byref(t), C.byref(h)), "dbgk_corr_table_stats")
        return int(t.value), int(h.value)

    def export_bits(self, first_byte=0, n_bytes=None):
        if n_bytes is None:
            n_bytes = max(4 ** self.k // 8, 1) - first_byte
        out = np.empty(n_bytes, dtype=np.uint8)
        _chk(lib().dbgk_corr_export_bits(self._h, first_byte, n_bytes, out.ctypes.data), "dbgk_corr_export_bits")
        return out

    def correct(self, bases, offsets):
        """-> (corrected bases: every read untrimmed at its input offset, records CORR_REC_DTYPE[n])"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.empty(max(bases.size, 1), dtype=np.uint8)
        rec = np.zeros(max(n, 1), dtype=CORR_REC_DTYPE)
        _chk(lib().dbgk_corr_reads(self._h, bases.ctypes.data, offsets.ctypes.data, n, out.ctypes.data, rec.ctypes.data),
             "dbgk_corr_reads")
        return out[:bases.size], rec[:n]

    def correct_device(self, d_bases, offsets):
        """correct() for bases already on the device (pointer, 16-byte aligned; offsets on the host) -> records; the corrected
        bytes stay on the device for compact()"""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        rec = np.zeros(max(n, 1), dtype=CORR_REC_DTYPE)
        _chk(lib().dbgk_corr_reads_device(self._h, d_bases, offsets.ctypes.data, n, rec.ctypes.data), "dbgk_corr_reads_device")
        return rec[:n]

    @staticmethod
    def _info(info):
        return {f: getattr(info, f) for f, _ in CorrCompactInfo._fields_}

    def compact(self):
        """the last batch trimmed and packed back to back on the device -> the counters and device times (dbgk_corr_compact_info)"""
        info = CorrCompactInfo()
        _chk(lib().dbgk_corr_compact(self._h, C.byref(info)), "dbgk_corr_compact")
        return self._info(info)

    def compact_from(self, bases, offsets, recs):
        """compact() of a batch held on the host: what correct() returned (untrimmed bytes, offsets, records)"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        recs = np.ascontiguousarray(recs, dtype=CORR_REC_DTYPE)
        n = len(offsets) - 1
        if len(recs) != n or int(offsets[-1]) > bases.size:
            raise ValueError("one record per read, and the last offset inside the bases")
        info = CorrCompactInfo()
        _chk(lib().dbgk_corr_compact_from(self._h, bases.ctypes.data, offsets.ctypes.data, recs.ctypes.data, n, C.byref(info)),
             "dbgk_corr_compact_from")
        return self._info(info)

    def compact_device(self):
        """-> (device pointer of the compact bases, device pointer of the n + 1 offsets, reads, bases)"""
        b, o, n, nb = _vp(), _vp(), _u64(), _u64()
        _chk(lib().dbgk_corr_compact_device(self._h, C.byref(b), C.byref(o), C.byref(n), C.byref(nb)), "dbgk_corr_compact_device")
        return b.value, o.value, int(n.value), int(nb.value)

    def compact_to_host(self):
        """-> (compact bases uint8, offsets uint64[n + 1])"""
        _, _, n, nb = self.compact_device()
        bases = np.empty(max(nb, 1), dtype=np.uint8)
        offsets = np.empty(n + 1, dtype=np.uint64)
        _chk(lib().dbgk_corr_compact_results(self._h, bases.ctypes.data, offsets.ctypes.data), "dbgk_corr_compact_results")
        return bases[:nb], offsets

    def annotate(self):
        """the annotation of every header of the compact batch, composed on the device -> (suffix bytes uint8, offsets uint64[n + 1]);
        the counters and device times (dbgk_corr_annot_info) are kept in `annot_info`"""
        info = CorrAnnotInfo()
        _chk(lib().dbgk_corr_annot(self._h, C.byref(info)), "dbgk_corr_annot")
        self.annot_info = {f: getattr(info, f) for f, _ in CorrAnnotInfo._fields_}
        suffix = np.empty(max(info.suffix_bytes, 1), dtype=np.uint8)
        offsets = np.empty(info.n + 1, dtype=np.uint64)
        _chk(lib().dbgk_corr_annot_results(self._h, suffix.ctypes.data, offsets.ctypes.data), "dbgk_corr_annot_results")
        return suffix[:info.suffix_bytes], offsets

    def annotate_device(self):
        """annotate() without the read-back -> DeviceSuffixes(device pointer of the suffix bytes, of the n + 1 offsets, records,
        bytes), what Formatter.format_device takes as `suffixes`"""
        info = CorrAnnotInfo()
        _chk(lib().dbgk_corr_annot(self._h, C.byref(info)), "dbgk_corr_annot")
        self.annot_info = {f: getattr(info, f) for f, _ in CorrAnnotInfo._fields_}
        s, o, n, nb = _vp(), _vp(), _u64(), _u64()
        _chk(lib().dbgk_corr_annot_device(self._h, C.byref(s), C.byref(o), C.byref(n), C.byref(nb)), "dbgk_corr_annot_device")
        return DeviceSuffixes(s.value, o.value, int(n.value), int(nb.value))

    def batch_stats(self):
        s = CorrStats()
        _chk(lib().dbgk_corr_batch_stats(self._h, C.byref(s)), "dbgk_corr_batch_stats")
        return {f: getattr(s, f) for f, _ in CorrStats._fields_}

    def mutation_scan(self, bases, offsets, skip):
        """simulate_lowfreq_kmer's scan -> np.uint64[k + 1]: bin j = mutated sites with j of their k windows absent"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError("offsets needs at least one entry (n + 1 entries for n sequences)")
        if int(offsets[-1]) > bases.size:
            raise ValueError("the last offset lies beyond the bases")
        if not 0 <= int(skip) < 1 << 32:
            raise ValueError("skip must fit in 32 bits (1 .. 2^32 - 1)")
        hist = np.zeros(self.k + 1, dtype=np.uint64)
        _chk(lib().dbgk_corr_mutation_scan(self._h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, int(skip), hist.ctypes.data),
             "dbgk_corr_mutation_scan")
        return hist

    def mutation_scan_ms(self):
        """device ms of the scan kernel of the last mutation_scan"""
        ms = C.c_double()
        _chk(lib().dbgk_corr_mutation_scan_ms(self._h, C.byref(ms)), "dbgk_corr_mutation_scan_ms")
        return ms.value


def concat_sequences(seqs):
    """a list of bytes / str -> (uint8 bases back to back, uint64 offsets[n + 1])"""
    seqs = [q.encode() if isinstance(q, str) else bytes(q) for q in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        offsets[1:] = np.cumsum([len(q) for q in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), offsets


class Mapper(_Handle):
    """map_reads / map_pair on the GPU (MAP section of include/dbgk.h).  Defaults are the reference's.  set_contigs builds the
    seed index and keeps the contig text on the device; map(bases, offsets) returns two hits per read (the second one only
    with second_alignment, the map_reads mode)."""
    _destroy = "dbgk_map_destroy"

    def __init__(self, k=31, s=5, r=250, identity=0.97, second_alignment=False, device=0):
        self._h = C.c_void_p()
        _chk(lib().dbgk_map_create(C.byref(MapParams(k, s, r, 1 if second_alignment else 0, identity)), device, C.byref(self._h)),
             "dbgk_map_create")

    def set_contigs(self, contigs):
        """a list of sequences (bytes / str); empty ones keep their index"""
        bases, offsets = concat_sequences(contigs)
        _chk(lib().dbgk_map_set_contigs(self._h, bases.ctypes.data if bases.size else None, offsets.ctypes.data, len(offsets) - 1),
             "dbgk_map_set_contigs")

    def set_ramp(self, first_chunk):
        _chk(lib().dbgk_map_set_ramp(self._h, first_chunk), "dbgk_map_set_ramp")

    def map(self, bases, offsets):
        """-> MAP_HIT_DTYPE[n, 2]"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        hits = np.zeros((max(n, 1), 2), dtype=MAP_HIT_DTYPE)
        _chk(lib().dbgk_map_reads(self._h, bases.ctypes.data if bases.size else None, offsets.ctypes.data, n, hits.ctypes.data),
             "dbgk_map_reads")
        return hits[:n]

    def map_device(self, d_bases, d_offsets, n_reads, n_bases, max_len, keep=False):
        """map() for a batch on the device, offsets included (pointers; Pairer.device, Corrector / Cleaner.compact_device); max_len
        is at least the longest read (PairInfo.max_len) -> MAP_HIT_DTYPE[n, 2].  keep: the hits stay on the device (hits_device,
        RowWriter.take_hits) and None is returned"""
        if keep:
            _chk(lib().dbgk_map_reads_device_keep(self._h, d_bases, d_offsets, n_reads, n_bases, max_len), "dbgk_map_reads_device_keep")
            return None
        hits = np.zeros((max(n_reads, 1), 2), dtype=MAP_HIT_DTYPE)
        _chk(lib().dbgk_map_reads_device(self._h, d_bases, d_offsets, n_reads, n_bases, max_len, hits.ctypes.data), "dbgk_map_reads_device")
        return hits[:n_reads]

    def hits_device(self):
        """-> (device pointer of the 2 n hits of the last batch, or None for an empty one; n)"""
        p, n = _vp(), _u64()
        _chk(lib().dbgk_map_hits_device(self._h, C.byref(p), C.byref(n)), "dbgk_map_hits_device")
        return p.value, int(n.value)

    def map_sequences(self, reads):
        return self.map(*concat_sequences(reads))

    def batch_stats(self):
        s = MapStats()
        _chk(lib().dbgk_map_batch_stats(self._h, C.byref(s)), "dbgk_map_batch_stats")
        return {f: getattr(s, f) for f, _ in MapStats._fields_}


class Pairer(_Handle):
    """The pair split on the GPU (PAIR section of include/dbgk.h): two batches of n reads, mate 1 and mate 2 of pair i at index i,
    become the PAIRED batch (both mates of every pair with two reads left) and the SINGLE batch (the mate that is left of every
    other pair).  split / split_device return the counters; results(which) and device(which) give either output."""
    _destroy = "dbgk_pair_destroy"

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _chk(lib().dbgk_pair_create(device, C.byref(self._h)), "dbgk_pair_create")

    @staticmethod
    def _info(info):
        return {f: getattr(info, f) for f, _ in PairInfo._fields_}

    def split(self, b1, o1, b2, o2, q1=None, q2=None):
        """two batches held on the host (bases uint8, offsets uint64[n + 1] from 0; qualities for both or for neither)"""
        if (q1 is None) != (q2 is None):
            raise ValueError("qualities for both batches or for neither")
        planes = []
        for b, o, q in ((b1, o1, q1), (b2, o2, q2)):
            b = np.ascontiguousarray(b, dtype=np.uint8)
            o = np.ascontiguousarray(o, dtype=np.uint64)
            q = None if q is None else np.ascontiguousarray(q, dtype=np.uint8)
            if len(o) < 1 or int(o[-1]) > b.size or (q is not None and q.size != b.size):
                raise ValueError("the last offset inside the bases, and as many qualities as bases")
            planes.append((b, o, q))
        (b1, o1, q1), (b2, o2, q2) = planes
        if len(o1) != len(o2):
            raise ValueError("both batches hold one read per pair")
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        # (a quality plane of no bytes is still a quality plane: the library tells the two apart by the pointer)
        none = np.zeros(16, dtype=np.uint8)
        qp = lambda q: None if q is None else (q.ctypes.data if q.size else none.ctypes.data)
        info = PairInfo()
        _chk(lib().dbgk_pair_split_from(self._h, ptr(b1), qp(q1), o1.ctypes.data, ptr(b2), qp(q2), o2.ctypes.data, len(o1) - 1, C.byref(info)),
             "dbgk_pair_split_from")
        return self._info(info)

    def split_device(self, d_b1, d_o1, d_b2, d_o2, n, d_q1=None, d_q2=None):
        """two batches on the device, offsets included (pointers; the planes 16-byte aligned) -- what compact_device of two
        Corrector / Cleaner handles returns"""
        info = PairInfo()
        _chk(lib().dbgk_pair_split_device(self._h, d_b1, d_q1, d_o1, d_b2, d_q2, d_o2, n, C.byref(info)), "dbgk_pair_split_device")
        return self._info(info)

    def device(self, which):
        """-> (device pointer of the bases, of the qualities or None, of the n + 1 offsets, reads, bases) of one output"""
        b, q, o, n, nb = _vp(), _vp(), _vp(), _u64(), _u64()
        _chk(lib().dbgk_pair_device(self._h, which, C.byref(b), C.byref(q), C.byref(o), C.byref(n), C.byref(nb)), "dbgk_pair_device")
        return b.value, q.value, o.value, int(n.value), int(nb.value)

    def results(self, which):
        """-> (bases uint8, qualities uint8 or None, offsets uint64[n + 1], source ids uint32[n]: 2 * pair + mate) of one output"""
        _, q, _, n, nb = self.device(which)
        bases = np.empty(max(nb, 1), dtype=np.uint8)
        quals = np.empty(max(nb, 1), dtype=np.uint8) if q else None
        offsets = np.empty(n + 1, dtype=np.uint64)
        ids = np.empty(max(n, 1), dtype=np.uint32)
        _chk(lib().dbgk_pair_results(self._h, which, bases.ctypes.data, quals.ctypes.data if q else None, offsets.ctypes.data, ids.ctypes.data),
             "dbgk_pair_results")
        return bases[:nb], (quals[:nb] if q else None), offsets, ids[:n]


class Parser(_Handle):
    """FASTQ (fmt 1) / FASTA (fmt 2) text parsed on the GPU (PARSE section of include/dbgk.h): a chunk of the file's bytes becomes the
    compact batch -- bases, qualities with with_quals, n + 1 offsets -- that the other stages read in place.  chunk / chunk_device
    return the counters and `consumed`; results() and device() give the batch; stream() feeds a file chunk by chunk."""
    _destroy = "dbgk_parse_destroy"

    def __init__(self, fmt, with_quals=False, device=0):
        self._h = C.c_void_p()
        _chk(lib().dbgk_parse_create(fmt, 1 if with_quals else 0, device, C.byref(self._h)), "dbgk_parse_create")

    @staticmethod
    def _info(info):
        return {f: getattr(info, f) for f, _ in ParseInfo._fields_}

    def chunk(self, text, last=True):
        """one chunk of text held on the host (bytes, or a uint8 array); last: the input ends with it"""
        a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        info = ParseInfo()
        _chk(lib().dbgk_parse_chunk(self._h, a.ctypes.data if a.size else None, a.size, 1 if last else 0, C.byref(info)), "dbgk_parse_chunk")
        return self._info(info)

    def chunk_device(self, d_text, n_bytes, last=True):
        """one chunk on the device (pointer, 16-byte aligned, readable up to n_bytes rounded up to 16), read in place"""
        info = ParseInfo()
        _chk(lib().dbgk_parse_chunk_device(self._h, d_text, n_bytes, 1 if last else 0, C.byref(info)), "dbgk_parse_chunk_device")
        return self._info(info)

    def stream(self, fileobj, chunk_bytes):
        """the text of fileobj (opened in binary mode) in chunks of chunk_bytes, each with what the chunk before it left unconsumed
        in front -> yields the info of every chunk; between two of them the batch of the chunk is results() / device()"""
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes >= 1")
        carry, block = b"", fileobj.read(chunk_bytes)
        while True:
            ahead = fileobj.read(chunk_bytes) if block else b""
            text = carry + block
            info = self.chunk(text, last=not ahead)
            yield info
            if not ahead:
                return
            carry, block = text[info["consumed"]:], ahead

    def device(self):
        """-> (device pointer of the bases, of the qualities or None, of the n + 1 offsets, reads, bases)"""
        b, q, o, n, nb = _vp(), _vp(), _vp(), _u64(), _u64()
        _chk(lib().dbgk_parse_device(self._h, C.byref(b), C.byref(q), C.byref(o), C.byref(n), C.byref(nb)), "dbgk_parse_device")
        return b.value, q.value, o.value, int(n.value), int(nb.value)

    def results(self):
        """-> (bases uint8, qualities uint8 or None, offsets uint64[n + 1], records PARSE_REC_DTYPE[n])"""
        _, q, _, n, nb = self.device()
        bases = np.empty(max(nb, 1), dtype=np.uint8)
        quals = np.empty(max(nb, 1), dtype=np.uint8) if q else None
        offsets = np.empty(n + 1, dtype=np.uint64)
        recs = np.empty(max(n, 1), dtype=PARSE_REC_DTYPE)
        _chk(lib().dbgk_parse_results(self._h, bases.ctypes.data, quals.ctypes.data if q else None, offsets.ctypes.data, recs.ctypes.data),
             "dbgk_parse_results")
        return bases[:nb], (quals[:nb] if q else None), offsets, recs[:n]


class Formatter(_Handle):
    """A compact batch written as FASTQ (fmt 1) / FASTA (fmt 2) text on the GPU (FORMAT section of include/dbgk.h): the headers from the
    text the parser parsed, the reads from the planes of a compact batch, an optional suffix per header from the host or, for
    format_device, from a plane on the device (DeviceSuffixes).  marker: 0,
    or the byte that replaces the first byte of every header.  format / format_device return the info as a dict (also kept in
    `info`); results() and device() give the text."""
    _destroy = "dbgk_fmt_destroy"

    def __init__(self, fmt, marker=0, device=0):
        self._h = C.c_void_p()
        self.info = None
        if isinstance(marker, (bytes, str)):
            marker = ord(marker)
        _chk(lib().dbgk_fmt_create(fmt, marker, device, C.byref(self._h)), "dbgk_fmt_create")

    @staticmethod
    def _suffix_plane(suffixes, n):
        """None, a list of n bytes objects, or (uint8 bytes, uint64 offsets[n + 1]) -> the two arrays, or (None, None)"""
        if suffixes is None:
            return None, None
        if isinstance(suffixes, tuple):
            data, off = suffixes
            return np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
        if len(suffixes) != n:
            raise ValueError("one suffix per record")
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(x) for x in suffixes], out=off[1:])
        return np.frombuffer(b"".join(suffixes), dtype=np.uint8), off

    def _done(self, info):
        self.info = {f: getattr(info, f) for f, _ in FmtInfo._fields_}
        return self.info

    def format(self, text, recs, bases, quals, offsets, suffixes=None):
        """everything held on the host: the text (bytes, or a uint8 array), PARSE_REC_DTYPE[n], the planes (quals None for FASTA)
        and uint64 offsets[n + 1]; suffixes as _suffix_plane takes them"""
        t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        recs = np.ascontiguousarray(recs, dtype=PARSE_REC_DTYPE)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(recs)
        if len(offsets) != n + 1:
            raise ValueError("n + 1 offsets")
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = None if quals is None else np.ascontiguousarray(quals, dtype=np.uint8)
        pad = np.zeros(1, dtype=np.uint8)  # (a plane of no bytes still says whether there is one)
        sd, so = self._suffix_plane(suffixes, n)
        info = FmtInfo()
        _chk(lib().dbgk_fmt_records(self._h, t.ctypes.data if t.size else None, t.size, recs.ctypes.data if n else None,
                                    (bases if bases.size else pad).ctypes.data, None if quals is None else (quals if quals.size else pad).ctypes.data,
                                    offsets.ctypes.data, n, sd.ctypes.data if sd is not None and sd.size else None,
                                    so.ctypes.data if so is not None else None, C.byref(info)), "dbgk_fmt_records")
        return self._done(info)

    def format_device(self, source, planes, suffixes=None):
        """source: a Parser after a chunk (its text and records where they lie), (parser, d_text, n_text) -- a Parser and the chunk
        its last chunk_device parsed -- or the pointers (d_text, n_text, d_recs) themselves; planes: (d_bases, d_quals or None, d_offsets, n) as the device() of a Parser, Cleaner, Corrector or
        Pairer gives them (further entries are ignored); suffixes as _suffix_plane takes them, or a DeviceSuffixes (a plane in device
        memory, what Corrector.annotate_device returns)"""
        if isinstance(source, Parser):   # the chunk of its last call, where chunk() uploaded it or chunk_device() read it
            d_text, nt = _vp(), _u64()
            _chk(lib().dbgk_parse_text_device(source._h, C.byref(d_text), C.byref(nt)), "dbgk_parse_text_device")
            source = (source, d_text.value, int(nt.value))
        if isinstance(source[0], Parser):
            parser, d_text, nt = source
            d_recs = _vp()
            _chk(lib().dbgk_parse_recs_device(parser._h, C.byref(d_recs)), "dbgk_parse_recs_device")
            d_recs = d_recs.value
        else:
            d_text, nt, d_recs = source
        d_bases, d_quals, d_off, n = planes[:4]
        info = FmtInfo()
        if isinstance(suffixes, DeviceSuffixes):   # a plane on the device, read where it lies
            _chk(lib().dbgk_fmt_records_device_suffix(self._h, d_text, nt, d_recs, d_bases, d_quals, d_off, n, suffixes.d_suffix, suffixes.d_offsets,
                                                      C.byref(info)), "dbgk_fmt_records_device_suffix")
            return self._done(info)
        sd, so = self._suffix_plane(suffixes, n)
        _chk(lib().dbgk_fmt_records_device(self._h, d_text, nt, d_recs, d_bases, d_quals, d_off, n,
                                           sd.ctypes.data if sd is not None and sd.size else None, so.ctypes.data if so is not None else None,
                                           C.byref(info)), "dbgk_fmt_records_device")
        return self._done(info)

    def device(self):
        """-> (device pointer of the text of the last call, its bytes)"""
        p, n = _vp(), _u64()
        _chk(lib().dbgk_fmt_device(self._h, C.byref(p), C.byref(n)), "dbgk_fmt_device")
        return p.value, int(n.value)

    def results(self):
        """-> the text of the last call as bytes"""
        _, n = self.device()
        out = np.empty(max(n, 1), dtype=np.uint8)
        _chk(lib().dbgk_fmt_results(self._h, out.ctypes.data, n), "dbgk_fmt_results")
        return out[:n].tobytes()


class RowWriter(_Handle):
    """The lines of map_reads' / map_pair's output files composed on the GPU (ROWS section of include/dbgk.h).  mode MAPROW_READS: one
    side, hits 2 i and 2 i + 1 the two alignments of read i; MAPROW_PAIR: two sides, read i of each a pair.  delims: the delimiter set of
    the read id.  set_contigs gives the table the rows print from; rows (everything on the host) and rows_device (a Parser's batch and
    hits taken from a Mapper with take_hits) return the info as a dict, also kept in `info`; results(stream) / device(stream) give the
    text of stream 0 .. 2."""
    _destroy = "dbgk_maprow_destroy"

    def __init__(self, mode, delims, min_read_len=0, device=0):
        self._h = C.c_void_p()
        self.info = None
        if isinstance(delims, str):
            delims = delims.encode("latin-1")
        self.n_sides = 2 if mode == MAPROW_PAIR else 1
        _chk(lib().dbgk_maprow_create(mode, delims, min_read_len, device, C.byref(self._h)), "dbgk_maprow_create")

    def set_contigs(self, names, lengths):
        """names: a list of bytes / str, the id of every contig; lengths: the length every row of that contig prints"""
        data, off = concat_sequences(names)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if len(lengths) != len(off) - 1:
            raise ValueError("one length per contig")
        _chk(lib().dbgk_maprow_set_contigs(self._h, data.ctypes.data if data.size else None, off.ctypes.data,
                                           lengths.ctypes.data if lengths.size else None, len(lengths)), "dbgk_maprow_set_contigs")

    def take_hits(self, side, mapper):
        """the hits of the Mapper's last batch, device to device, as side 0 or 1 of the next rows_device"""
        _chk(lib().dbgk_maprow_take_hits(self._h, side, mapper._h), "dbgk_maprow_take_hits")

    def _done(self, info):
        self.info = {"n": int(info.n), "counters": [int(v) for v in info.counters], "stream_bytes": [int(v) for v in info.stream_bytes],
                     "unprintable": int(info.unprintable), "ms_scan": info.ms_scan, "ms_write": info.ms_write}
        return self.info

    def rows(self, sides, n=None):
        """sides: per side (text, recs PARSE_REC_DTYPE[n], bases, offsets uint64[n + 1], hits MAP_HIT_DTYPE[n, 2]), all on the host"""
        if len(sides) != self.n_sides:
            raise ValueError("one side for READS, two for PAIR")
        keep, arr = [], (MapRowSide * self.n_sides)()
        pad = np.zeros(16, dtype=np.uint8)
        for s, (text, recs, bases, offsets, hits) in enumerate(sides):
            t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
            recs = np.ascontiguousarray(recs, dtype=PARSE_REC_DTYPE)
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            hits = np.ascontiguousarray(hits, dtype=MAP_HIT_DTYPE).reshape(-1)
            m = len(offsets) - 1
            if n is None:
                n = m
            if m != n or len(recs) != n or hits.size != 2 * n:
                raise ValueError("n records, n + 1 offsets and 2 n hits per side")
            keep.append((t, recs, bases, offsets, hits))
            arr[s] = MapRowSide(t.ctypes.data if t.size else None, t.size, (recs if n else pad).ctypes.data, (bases if bases.size else pad).ctypes.data,
                                offsets.ctypes.data, (hits if n else pad).ctypes.data)
        info = MapRowInfo()
        _chk(lib().dbgk_maprow_rows(self._h, arr, n, C.byref(info)), "dbgk_maprow_rows")
        return self._done(info)

    def rows_device(self, sides, n):
        """sides: per side a Parser after a chunk, or the pointers (d_text, n_text, d_recs, d_bases, d_offsets); the hits are those of
        take_hits"""
        if len(sides) != self.n_sides:
            raise ValueError("one side for READS, two for PAIR")
        arr = (MapRowSide * self.n_sides)()
        for s, side in enumerate(sides):
            if isinstance(side, Parser):
                d_text, nt, d_recs = _vp(), _u64(), _vp()
                _chk(lib().dbgk_parse_text_device(side._h, C.byref(d_text), C.byref(nt)), "dbgk_parse_text_device")
                _chk(lib().dbgk_parse_recs_device(side._h, C.byref(d_recs)), "dbgk_parse_recs_device")
                d_bases, _, d_off, _, _ = side.device()
                side = (d_text.value, int(nt.value), d_recs.value, d_bases, d_off)
            arr[s] = MapRowSide(side[0], side[1], side[2], side[3], side[4], None)
        info = MapRowInfo()
        _chk(lib().dbgk_maprow_rows_device(self._h, arr, n, C.byref(info)), "dbgk_maprow_rows_device")
        return self._done(info)

    def device(self, stream):
        """-> (device pointer of the text of a stream of the last call, its bytes)"""
        p, n = _vp(), _u64()
        _chk(lib().dbgk_maprow_device(self._h, stream, C.byref(p), C.byref(n)), "dbgk_maprow_device")
        return p.value, int(n.value)

    def results(self, stream):
        """-> the text of a stream of the last call as bytes"""
        _, n = self.device(stream)
        out = np.empty(max(n, 1), dtype=np.uint8)
        _chk(lib().dbgk_maprow_results(self._h, stream, out.ctypes.data, n), "dbgk_maprow_results")
        return out[:n].tobytes()


class Deflater(_Handle):
    """bytes deflated on the GPU into BGZF-framed gzip members (GZ section of include/dbgk.h): level 0 stored, 1 one dynamic-Huffman
    block of literals per member, 2 one over LZ77 tokens.  deflate / deflate_device return the members of the call as bytes; `info` holds the counters of
    the last call; stream() compresses a file window by window."""
    _destroy = "dbgk_gz_destroy"

    def __init__(self, level=GZ_MAX_LEVEL):
        self._h = C.c_void_p()
        self.info = None
        _chk(lib().dbgk_gz_create(level, C.byref(self._h)), "dbgk_gz_create")

    def _done(self, info):
        self.info = {f: getattr(info, f) for f, _ in GzInfo._fields_}
        return self.results()

    def deflate(self, data, last=True):
        """text held on the host (bytes, or a uint8 array) -> its members, with the end marker behind them if last"""
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        info = GzInfo()
        _chk(lib().dbgk_gz_deflate(self._h, a.ctypes.data if a.size else None, a.size, 1 if last else 0, C.byref(info)), "dbgk_gz_deflate")
        return self._done(info)

    def deflate_device(self, d_text, n, last=True):
        """text on the device (pointer, 16-byte aligned, readable up to n rounded up to 16), read in place"""
        info = GzInfo()
        _chk(lib().dbgk_gz_deflate_device(self._h, d_text, n, 1 if last else 0, C.byref(info)), "dbgk_gz_deflate_device")
        return self._done(info)

    def device(self):
        """-> (device pointer of the members of the last call or None, their bytes)"""
        p, n = _vp(), _u64()
        _chk(lib().dbgk_gz_device(self._h, C.byref(p), C.byref(n)), "dbgk_gz_device")
        return p.value, int(n.value)

    def results(self):
        """-> the members of the last call as bytes"""
        _, n = self.device()
        out = np.empty(max(n, 1), dtype=np.uint8)
        _chk(lib().dbgk_gz_results(self._h, out.ctypes.data, n), "dbgk_gz_results")
        return out[:n].tobytes()

    def timing(self):
        t = GzTiming()
        _chk(lib().dbgk_gz_timing_get(self._h, C.byref(t)), "dbgk_gz_timing_get")
        return {f: getattr(t, f) for f, _ in GzTiming._fields_}

    def stream(self, src, dst, chunk_bytes):
        """src (opened in binary mode) read in windows of chunk_bytes, the members of every window written to dst, the end marker
        once behind the last -> the summed counters"""
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes >= 1")
        total = {f: 0 for f, _ in GzInfo._fields_}
        block = src.read(chunk_bytes)
        while True:
            ahead = src.read(chunk_bytes) if block else b""
            dst.write(self.deflate(block, last=not ahead))
            for f in total:
                total[f] += self.info[f]
            if not ahead:
                return total
            block = ahead


class Inflater(_Handle):
    """BGZF-framed gzip members inflated on the GPU (INFLATE section of include/dbgk.h).  inflate / inflate_device return the bytes
    of the members of the call and its counters; a member that is refused leaves zeros, `info["n_bad"]` counts them and member_status()
    says why; device() is the text where it lies, for Parser.chunk_device; stream() inflates a file window by window."""
    _destroy = "dbgk_inf_destroy"

    def __init__(self, max_out_bytes=0):
        self._h = C.c_void_p()
        self.info = None
        _chk(lib().dbgk_inf_create(max_out_bytes, C.byref(self._h)), "dbgk_inf_create")

    def _done(self, info):
        self.info = {f: getattr(info, f) for f, _ in InfInfo._fields_}
        return self.results(), self.info

    def inflate(self, data, last=True):
        """members held on the host (bytes, or a uint8 array) -> (their bytes, info); with last=False a member cut short at the end
        is left unconsumed: info["consumed"]"""
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        info = InfInfo()
        _chk(lib().dbgk_inf_inflate(self._h, a.ctypes.data if a.size else None, a.size, 1 if last else 0, C.byref(info)), "dbgk_inf_inflate")
        return self._done(info)

    def inflate_device(self, d_gz, offsets, n_bytes=None):
        """members on the device: d_gz a pointer (16-byte aligned) or a uint8 torch tensor; offsets: where each member starts and,
        last, where the last one ends.  n_bytes: the buffer's size (a tensor's own by default, else the last offset)"""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.size < 1:
            raise ValueError("n_members + 1 offsets")
        if hasattr(d_gz, "data_ptr"):
            n_bytes = d_gz.numel() if n_bytes is None else n_bytes
            d_gz = d_gz.data_ptr()
        n_bytes = int(off[-1]) if n_bytes is None else n_bytes
        info = InfInfo()
        _chk(lib().dbgk_inf_inflate_device(self._h, d_gz, n_bytes, off.ctypes.data_as(C.POINTER(_u64)), off.size - 1, C.byref(info)), "dbgk_inf_inflate_device")
        return self._done(info)

    def device_ptr(self):
        """-> (device pointer of the text of the last call or None, its bytes)"""
        p, n = _vp(), _u64()
        _chk(lib().dbgk_inf_device(self._h, C.byref(p), C.byref(n)), "dbgk_inf_device")
        return p.value, int(n.value)

    def device(self):
        """-> the text of the last call as a uint8 torch tensor that views the handle's memory (valid until the next call): 16-byte
        aligned and readable up to its size rounded up to 16, so Parser.chunk_device(t.data_ptr(), t.numel()) reads it in place"""
        import torch
        p, n = self.device_ptr()
        if not n:
            return torch.empty(0, dtype=torch.uint8, device="cuda")

        class _View:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (p, False), "version": 2}
        t = torch.as_tensor(_View(), device="cuda")
        t._dbgk_owner = self
        return t

    def results(self):
        """-> the text of the last call as bytes"""
        _, n = self.device_ptr()
        out = np.empty(max(n, 1), dtype=np.uint8)
        _chk(lib().dbgk_inf_results(self._h, out.ctypes.data, n), "dbgk_inf_results")
        return out[:n].tobytes()

    def member_status(self):
        """-> one verdict per member of the last call (uint8; names in INF_REASONS)"""
        n = self.info["n_members"] if self.info else 0
        out = np.zeros(max(n, 1), dtype=np.uint8)
        _chk(lib().dbgk_inf_member_status(self._h, out.ctypes.data, n), "dbgk_inf_member_status")
        return out[:n]

    def timing(self):
        t = InfTiming()
        _chk(lib().dbgk_inf_timing_get(self._h, C.byref(t)), "dbgk_inf_timing_get")
        return {f: getattr(t, f) for f, _ in InfTiming._fields_}

    def stream(self, fileobj, window):
        """the members of fileobj (opened in binary mode) in windows of `window` bytes, each with what the window before it left
        unconsumed in front -> yields (bytes, info) per window; a tail that is no whole member at the end of the file is an error"""
        if window < 1:
            raise ValueError("window >= 1")
        carry, block = b"", fileobj.read(window)
        while True:
            ahead = fileobj.read(window) if block else b""
            data = carry + block
            text, info = self.inflate(data, last=not ahead)
            yield text, info
            if not ahead:
                return
            carry, block = data[info["consumed"]:], ahead


class Cleaner(_Handle):
    """clean_adapter / clean_lowqual on the GPU (CLEAN section of include/dbgk.h).  The device returns one hit / one block per
    read; trim_adapter and trim_lowqual cut the records the way the two programs do."""
    _destroy = "dbgk_clean_destroy"

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _chk(lib().dbgk_clean_create(device, C.byref(self._h)), "dbgk_clean_create")

    def set_adapters(self, adapters, score_cutoff=12):
        """contaminant sequences (bytes / str) in the order they are tried"""
        bases, offsets = concat_sequences(adapters)
        _chk(lib().dbgk_clean_set_adapters(self._h, bases.ctypes.data if bases.size else None, offsets.ctypes.data,
                                           len(offsets) - 1, score_cutoff), "dbgk_clean_set_adapters")

    def adapter(self, bases, offsets):
        """-> ADAPTER_HIT_DTYPE[n]"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        hits = np.zeros(max(n, 1), dtype=ADAPTER_HIT_DTYPE)
        _chk(lib().dbgk_clean_adapter(self._h, bases.ctypes.data if bases.size else None, offsets.ctypes.data, n, hits.ctypes.data),
             "dbgk_clean_adapter")
        return hits[:n]

    def lowqual(self, bases, quals, offsets, error_rate_cutoff=0.001, quality_shift=33):
        """bases and quals share the offsets -> LOWQUAL_BLOCK_DTYPE[n]"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if bases.size != quals.size:
            raise ValueError("bases and quals differ in size")
        n = len(offsets) - 1
        blocks = np.zeros(max(n, 1), dtype=LOWQUAL_BLOCK_DTYPE)
        _chk(lib().dbgk_clean_lowqual(self._h, bases.ctypes.data if bases.size else None, quals.ctypes.data if quals.size else None,
                                      offsets.ctypes.data, n, error_rate_cutoff, quality_shift, blocks.ctypes.data), "dbgk_clean_lowqual")
        return blocks[:n]

    def lowqual_device(self, d_bases, d_quals, offsets, error_rate_cutoff=0.001, quality_shift=33):
        """lowqual() for planes already on the device (pointers, 16-byte aligned, readable 16 bytes behind the last read; offsets on
        the host) -> LOWQUAL_BLOCK_DTYPE[n]; the planes are read again by compact()"""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        blocks = np.zeros(max(n, 1), dtype=LOWQUAL_BLOCK_DTYPE)
        _chk(lib().dbgk_clean_lowqual_device(self._h, d_bases, d_quals, offsets.ctypes.data, n, error_rate_cutoff, quality_shift,
                                             blocks.ctypes.data), "dbgk_clean_lowqual_device")
        return blocks[:n]

    def adapter_device(self, d_bases, d_quals, offsets):
        """adapter() for bases already on the device; d_quals (or None) only travels into the compact batch -> ADAPTER_HIT_DTYPE[n]"""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        hits = np.zeros(max(n, 1), dtype=ADAPTER_HIT_DTYPE)
        _chk(lib().dbgk_clean_adapter_device(self._h, d_bases, d_quals, offsets.ctypes.data, n, hits.ctypes.data),
             "dbgk_clean_adapter_device")
        return hits[:n]

    @staticmethod
    def _info(info):
        return {f: getattr(info, f) for f, _ in CleanCompactInfo._fields_}

    def compact(self, min_len=75):
        """the last batch cut as its program cuts it and packed back to back on the device -> the .stat counters and device times
        (dbgk_clean_compact_info)"""
        info = CleanCompactInfo()
        _chk(lib().dbgk_clean_compact(self._h, min_len, C.byref(info)), "dbgk_clean_compact")
        return self._info(info)

    def compact_from(self, kind, bases, quals, offsets, recs, quality_shift=33, min_len=75):
        """compact() of a batch held on the host: reads, qualities (or None) and the records of an earlier adapter() / lowqual();
        kind is CLEAN_KIND_ADAPTER or CLEAN_KIND_LOWQUAL"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = None if quals is None else np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        recs = np.ascontiguousarray(recs, dtype=LOWQUAL_BLOCK_DTYPE if kind == CLEAN_KIND_LOWQUAL else ADAPTER_HIT_DTYPE)
        n = len(offsets) - 1
        if len(recs) != n or int(offsets[-1]) > bases.size or (quals is not None and quals.size != bases.size):
            raise ValueError("one record per read, the last offset inside the bases, and as many qualities as bases")
        info = CleanCompactInfo()
        _chk(lib().dbgk_clean_compact_from(self._h, kind, bases.ctypes.data if bases.size else None,
                                           quals.ctypes.data if quals is not None and quals.size else None, offsets.ctypes.data,
                                           recs.ctypes.data if n else None, n, quality_shift, min_len, C.byref(info)), "dbgk_clean_compact_from")
        return self._info(info)

    def compact_device(self):
        """-> (device pointer of the compact bases, of the qualities or None, of the n + 1 offsets, reads, bases)"""
        b, q, o, n, nb = _vp(), _vp(), _vp(), _u64(), _u64()
        _chk(lib().dbgk_clean_compact_device(self._h, C.byref(b), C.byref(q), C.byref(o), C.byref(n), C.byref(nb)),
             "dbgk_clean_compact_device")
        return b.value, q.value, o.value, int(n.value), int(nb.value)

    def compact_to_host(self):
        """-> (compact bases uint8, compact qualities uint8 or None, offsets uint64[n + 1])"""
        _, q, _, n, nb = self.compact_device()
        bases = np.empty(max(nb, 1), dtype=np.uint8)
        quals = np.empty(max(nb, 1), dtype=np.uint8) if q else None
        offsets = np.empty(n + 1, dtype=np.uint64)
        _chk(lib().dbgk_clean_compact_results(self._h, bases.ctypes.data, quals.ctypes.data if q else None, offsets.ctypes.data),
             "dbgk_clean_compact_results")
        return bases[:nb], (quals[:nb] if q else None), offsets

    def batch_stats(self):
        s = CleanStats()
        _chk(lib().dbgk_clean_batch_stats(self._h, C.byref(s)), "dbgk_clean_batch_stats")
        return {f: getattr(s, f) for f, _ in CleanStats._fields_}

    def trim_adapter(self, records, adapter_ids, min_len=75):
        """records: (head, read, qual) as str; adapter_ids: the names of the sequences given to set_adapters.
        -> (records as bin/clean_adapter writes them, hits)"""
        hits = self.adapter(*concat_sequences([r[1] for r in records]))
        out = []
        for (head, read, qual), h in zip(records, hits.tolist()):
            a, score, rs, re, as_, ae = h
            if a >= 0:
                read, qual = read[:rs - 1], qual[:rs - 1]
                head += "   Aligned to adapter %s,  reads_pos: %d-%d, adapter_pos: %d-%d,   score: %d" % (adapter_ids[a], rs, re, as_, ae, score)
            if len(read) < min_len:
                read, qual, head = "", "", head + "   RemoveShort"
            out.append((head, read, qual))
        return out, hits

    def trim_lowqual(self, records, error_rate_cutoff=0.001, quality_shift=33, min_len=75):
        """-> (records as bin/clean_lowqual writes them, blocks)"""
        recs = [(h, s, q) if len(s) == len(q) else (h, "", "") for h, s, q in records]
        bases, offsets = concat_sequences([r[1] for r in recs])
        quals, _ = concat_sequences([r[2].encode("latin-1") for r in recs])
        blocks = self.lowqual(bases, quals, offsets, error_rate_cutoff, quality_shift)
        out = []
        for (head, read, qual), b in zip(recs, blocks.tolist()):
            err, start, length, trimmed, _ = b
            n = len(read)
            qual = "".join(chr(quality_shift) if c == "N" else q for c, q in zip(read, qual))
            head += "    RQ: " + ("%.17g" % (err / n * 100) if n else "-nan") + "%"
            if trimmed:
                head += "  TrimLowQual"
                read, qual = (read[start - 1:start - 1 + length], qual[start - 1:start - 1 + length]) if start else ("", "")
            if len(read) < min_len:
                read, qual, head = "", "", head + "  FilterShort"
            out.append((head, read, qual))
        return out, blocks


class _LinkTable(_Handle):
    """What Scaffolder, GapFiller and SuperLinker share: the handle, the contigs, the link table and the emit of the C calls that start with
    `_prefix` ("dbgk_link" / "dbgk_fill"); `_item_dtype` is the dtype of the items emit() takes."""
    _prefix = None
    _item_dtype = None
    _destroy = property(lambda self: self._prefix + "_destroy")

    def _call(self, name, *args, ok=(0,)):
        """lib().<_prefix>_<name>(handle, *args) -> its return code, checked under the C function's name unless it is in `ok`"""
        what = "%s_%s" % (self._prefix, name)
        rc = getattr(lib(), what)(self._h, *args)
        if rc not in ok:
            _chk(rc, what)
        return rc

    def set_contigs(self, lengths):
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        self._call("set_contigs", lengths.ctypes.data if lengths.size else None, len(lengths))
        self.n_contigs = len(lengths)
        self._lengths = lengths.tolist()

    def table(self):
        """-> first[2n + 2] (links of node i: links[first[i]:first[i + 1]] in chain order), LINK_ENTRY_DTYPE links, counters"""
        n, ctr = C.c_uint64(), LinkCounters()
        self._call("export", None, None, 0, C.byref(n), C.byref(ctr))
        first = np.zeros(2 * self.n_contigs + 2, dtype=np.uint64)
        links = np.zeros(max(n.value, 1), dtype=LINK_ENTRY_DTYPE)
        self._call("export", first.ctypes.data, links.ctypes.data, len(links), C.byref(n), C.byref(ctr))
        return first, links[:n.value], {"FR": ctr.fr, "RF": ctr.rf, "FF": ctr.ff, "RR": ctr.rr, "wrong": ctr.wrong}

    def snapshot(self, stage):
        """stage 0: links.all, 1: links.uniq -> inlink, link (uint8 per node), links (the table's shape, cleared entries zero)"""
        first, links, _ = self.table()
        inlink = np.zeros(2 * self.n_contigs + 1, dtype=np.uint8)
        link = np.zeros(2 * self.n_contigs + 1, dtype=np.uint8)
        e = np.zeros(max(len(links), 1), dtype=LINK_ENTRY_DTYPE)
        self._call("snapshot", stage, inlink.ctypes.data, link.ctypes.data, e.ctypes.data)
        return inlink, link, e[:len(links)]

    def links_text(self, stage):
        """the text of the program's *.links.all (stage 0) / *.links.uniq (stage 1)"""
        first = self.table()[0].tolist()
        inlink, link, e = self.snapshot(stage)
        t, f, z = e["target"].tolist(), e["freq"].tolist(), e["size"].tolist()
        out = ["ctg_id\tincoming_link_num\toutgoing_link_num\tlinked_id,pair_num,sum_size,avg_size;\n"]
        for i in range(1, 2 * self.n_contigs + 1):
            row = "%d\t%d\t%d" % (i, inlink[i], link[i])
            for j in range(first[i], first[i + 1]):
                if f[j] > 0:
                    avg = abs(z[j]) // f[j]
                    row += "\t%d,%d,%d,%d" % (t[j], f[j], z[j], -avg if z[j] < 0 else avg)
            out.append(row + "\n")
        return "".join(out)

    def emit(self, contigs, items):
        """the items back to back -> uint8 array.  A Scaffolder's item is a contig as it is, reverse-complemented, or a run of N; a
        GapFiller's a contig or its reverse complement, possibly cut, or the consensus bytes of a gap."""
        bases, offsets = contigs if isinstance(contigs, tuple) else concat_sequences(contigs)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        items = np.ascontiguousarray(items, dtype=self._item_dtype)
        n = C.c_uint64()
        args = (bases.ctypes.data if bases.size else None, offsets.ctypes.data, len(offsets) - 1,
                items.ctypes.data if len(items) else None, len(items))
        self._call("emit", *args, None, 0, C.byref(n), ok=(0, ERR_CAPACITY))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        if n.value:
            self._call("emit", *args, out.ctypes.data, n.value, C.byref(n))
        return out[:n.value]


class Scaffolder(_LinkTable):
    """link_scaffold on the GPU (LINK section of include/dbgk.h).  Defaults are the reference's.  Contig c is node 2c + 1, its
    reverse strand node 2c + 2.  set_contigs(lengths), add_pairs / add_hits in file order, build(), then table() for the links,
    resolve() for the reference's clean-up passes and walk, layout() and emit() for the scaffolds."""
    _prefix = "dbgk_link"
    _item_dtype = LINK_ITEM_DTYPE

    def __init__(self, mate_pair=0, pair_num_cut=3, insert_size=400, device=0):
        self._h = C.c_void_p()
        self.n_contigs = 0
        _chk(lib().dbgk_link_create(C.byref(LinkParams(mate_pair, pair_num_cut, insert_size)), device, C.byref(self._h)),
             "dbgk_link_create")

    def add_pairs(self, recs):
        """LINK_PAIR_DTYPE records (any structured array with its first eight fields), behind those added so far"""
        if recs.dtype != LINK_PAIR_DTYPE:
            r = np.zeros(len(recs), dtype=LINK_PAIR_DTYPE)
            for f in LINK_PAIR_DTYPE.names[:8]:
                r[f] = recs[f]
            recs = r
        recs = np.ascontiguousarray(recs)
        _chk(lib().dbgk_link_add_pairs(self._h, recs.ctypes.data if len(recs) else None, len(recs)), "dbgk_link_add_pairs")

    def add_hits(self, hits1, hits2):
        """what Mapper.map returned for the first and for the second mates (MAP_HIT_DTYPE[n, 2], or [n]: the first hits)"""
        h = []
        for x in (hits1, hits2):
            x = np.asarray(x, dtype=MAP_HIT_DTYPE)
            h.append(np.ascontiguousarray(x[:, 0] if x.ndim == 2 else x))
        if len(h[0]) != len(h[1]):
            raise ValueError("as many first mates as second mates")
        n = len(h[0])
        _chk(lib().dbgk_link_add_hits(self._h, h[0].ctypes.data if n else None, h[1].ctypes.data if n else None, n), "dbgk_link_add_hits")

    def build(self):
        _chk(lib().dbgk_link_build(self._h), "dbgk_link_build")

    def resolve(self):
        s = LinkSummary()
        _chk(lib().dbgk_link_resolve(self._h, C.byref(s)), "dbgk_link_resolve")
        return {f: getattr(s, f) for f, _ in LinkSummary._fields_}

    def layout(self):
        """-> scaf_first[scaffolds + 1], LINK_ITEM_DTYPE items, repeat contigs: in output order"""
        s = self.resolve()
        scaf_first = np.zeros(s["scaffolds"] + 1, dtype=np.uint64)
        items = np.zeros(max(s["items"], 1), dtype=LINK_ITEM_DTYPE)
        repeats = np.zeros(max(s["repeat_nodes"], 1), dtype=np.int32)
        _chk(lib().dbgk_link_layout(self._h, scaf_first.ctypes.data, items.ctypes.data, repeats.ctypes.data), "dbgk_link_layout")
        return scaf_first, items[:s["items"]], repeats[:s["repeat_nodes"]]

    def pos_tabs(self, names):
        """the texts of *.scaffold.pos.tab and *.scaffold_repeat.pos.tab"""
        scaf_first, items, repeats = self.layout()
        lens = self._lengths
        pos, sid = [], -1
        for s in range(len(scaf_first) - 1):
            sid += 2
            pos.append(">scf_%d\n" % sid)
            at = 0
            for c, v in items[int(scaf_first[s]):int(scaf_first[s + 1])].tolist():
                size = lens[c] if c >= 0 else v
                pos.append("\t%s\t%d\t%d\t%d\t%s\n" % (names[c] if c >= 0 else "gap", at + 1, at + size, size,
                                                        "N" if c < 0 else "R" if v else "F"))
                at += size
        rep = []
        for c in repeats.tolist():
            sid += 2
            rep.append(">scf_%d\n\t%s\t1\t%d\t%d\tF\n" % (sid, names[c], lens[c], lens[c]))
        return "".join(pos), "".join(rep)

    def batch_stats(self):
        s = LinkTiming()
        _chk(lib().dbgk_link_batch_stats(self._h, C.byref(s)), "dbgk_link_batch_stats")
        return {f: getattr(s, f) for f, _ in LinkTiming._fields_}


def float9(x):
    """boost::lexical_cast<string>(float): nine significant digits"""
    return "%.9g" % float(np.float32(x))


class GapFiller(_LinkTable):
    """link_contig on the GPU (FILL section of include/dbgk.h).  Contig c is node 2c + 1, its reverse strand node 2c + 2.
    set_contigs(lengths), set_reads(reads), add_records / add_hits in file order, build(), then table() and gap_stats(),
    resolve() for the passes, the walk and the gap consensus, layout() and emit() for the scafftigs."""
    _prefix = "dbgk_fill"
    _item_dtype = FILL_ITEM_DTYPE

    def __init__(self, pair_num_cut=3, device=0):
        self._h = C.c_void_p()
        self.n_contigs = 0
        _chk(lib().dbgk_fill_create(C.byref(FillParams(pair_num_cut, (C.c_int32 * 3)(0, 0, 0))), device, C.byref(self._h)), "dbgk_fill_create")

    def set_reads(self, reads):
        """a list of sequences (bytes / str), or (bases, offsets): the reads the records' `read` fields index"""
        bases, offsets = reads if isinstance(reads, tuple) else concat_sequences(reads)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _chk(lib().dbgk_fill_set_reads(self._h, bases.ctypes.data if bases.size else None, offsets.ctypes.data, len(offsets) - 1),
             "dbgk_fill_set_reads")

    def add_records(self, recs):
        """FILL_RECORD_DTYPE records (any structured array with its first eight fields), behind those added so far"""
        if recs.dtype != FILL_RECORD_DTYPE:
            r = np.zeros(len(recs), dtype=FILL_RECORD_DTYPE)
            for f in FILL_RECORD_DTYPE.names[:8]:
                r[f] = recs[f]
            recs = r
        recs = np.ascontiguousarray(recs)
        _chk(lib().dbgk_fill_add_records(self._h, recs.ctypes.data if len(recs) else None, len(recs)), "dbgk_fill_add_records")

    def add_hits(self, hits, first_read=0):
        """what Mapper.map (second_alignment) returned for reads first_read, first_read + 1, ...: MAP_HIT_DTYPE[n, 2]"""
        hits = np.ascontiguousarray(np.asarray(hits, dtype=MAP_HIT_DTYPE))
        if hits.ndim != 2 or hits.shape[1] != 2:
            raise ValueError("two hits per read")
        n = len(hits)
        _chk(lib().dbgk_fill_add_hits(self._h, hits.ctypes.data if n else None, n, first_read), "dbgk_fill_add_hits")

    def build(self):
        _chk(lib().dbgk_fill_build(self._h), "dbgk_fill_build")

    def gap_stats(self):
        """-> FILL_GAPSTAT_DTYPE per contig pair with a record, ascending by (contig_lo, contig_hi)"""
        n = C.c_uint64()
        _chk(lib().dbgk_fill_gap_stats(self._h, None, 0, C.byref(n)), "dbgk_fill_gap_stats")
        out = np.zeros(max(n.value, 1), dtype=FILL_GAPSTAT_DTYPE)
        _chk(lib().dbgk_fill_gap_stats(self._h, out.ctypes.data, len(out), C.byref(n)), "dbgk_fill_gap_stats")
        return out[:n.value]

    def resolve(self):
        s = FillSummary()
        _chk(lib().dbgk_fill_resolve(self._h, C.byref(s)), "dbgk_fill_resolve")
        return {f: getattr(s, f) for f, _ in FillSummary._fields_}

    def layout(self):
        """-> scaf_first[scafftigs + 1], FILL_ITEM_DTYPE items, FILL_GAP_DTYPE gaps, repeat contigs, consensus bytes: in output order"""
        s = self.resolve()
        scaf_first = np.zeros(s["scaffolds"] + 1, dtype=np.uint64)
        items = np.zeros(max(s["items"], 1), dtype=FILL_ITEM_DTYPE)
        gaps = np.zeros(max(s["gaps"], 1), dtype=FILL_GAP_DTYPE)
        repeats = np.zeros(max(s["repeat_nodes"], 1), dtype=np.int32)
        cons = np.zeros(max(s["cons_bytes"], 1), dtype=np.uint8)
        _chk(lib().dbgk_fill_layout(self._h, scaf_first.ctypes.data, items.ctypes.data, gaps.ctypes.data, repeats.ctypes.data, cons.ctypes.data),
             "dbgk_fill_layout")
        return scaf_first, items[:s["items"]], gaps[:s["gaps"]], repeats[:s["repeat_nodes"]], cons[:s["cons_bytes"]]

    def pos_tabs(self, names):
        """the texts of *.contig_R.pos.tab and *.contig_R.repeat.pos.tab"""
        scaf_first, items, gaps, repeats, _ = self.layout()
        lens = self._lengths
        pos = ["#scafftig_id\tblock_id\tblock_start\tblock_end\tblock_size\tdirection\tgapsize_mode_freq\tgapsize_total_freq\t"
               "gapsize_variance\tgapseq_identity\n"]
        sid = -1
        G = gaps.tolist()
        for s in range(len(scaf_first) - 1):
            sid += 2
            pos.append(">sct_%d\n" % sid)
            at = 0
            for c, rev, length, g, _ in items[int(scaf_first[s]):int(scaf_first[s + 1])].tolist():
                if c >= 0:
                    pos.append("\t%s\t%d\t%d\t%d\t%s\n" % (names[c], at + 1, at + length, length, "R" if rev else "F"))
                    at += length
                else:
                    mode, mf, tf, var, ident, _ = G[g]
                    if mode <= 0:
                        pos.append("\tgap\t%d\t%d\t%d\tN\t%d\t%d\t%d\n" % (at, at, mode, mf, tf, var))
                    else:
                        pos.append("\tgap\t%d\t%d\t%d\tN\t%d\t%d\t%d\t%s\n" % (at + 1, at + length, length, mf, tf, var, float9(ident)))
                        at += length
        rep = []
        for c in repeats.tolist():
            sid += 2
            rep.append(">sct_%d\n\t%s\t1\t%d\t%d\tF\n" % (sid, names[c], lens[c], lens[c]))
        return "".join(pos), "".join(rep)

    def timing(self):
        s = FillTiming()
        _chk(lib().dbgk_fill_batch_stats(self._h, C.byref(s)), "dbgk_fill_batch_stats")
        return {f: getattr(s, f) for f, _ in FillTiming._fields_}


class SuperLinker(_LinkTable):
    """link_supertig on the GPU (SUPER section of include/dbgk.h).  Contig c is node 2c + 1, its reverse strand node 2c + 2.
    set_contigs(lengths), set_reads(reads), add_records / add_hits in file order, build(), then table() and gap_stats(),
    resolve() for the passes, the walk and the slices of every gap, layout(), slices() and emit() for the super-contigs."""
    _prefix = "dbgk_super"
    _item_dtype = LINK_ITEM_DTYPE

    def __init__(self, pair_num_cut=3, device=0):
        self._h = C.c_void_p()
        self.n_contigs = 0
        _chk(lib().dbgk_super_create(C.byref(SuperParams(pair_num_cut, (C.c_int32 * 3)(0, 0, 0))), device, C.byref(self._h)), "dbgk_super_create")

    def set_reads(self, reads):
        """a list of sequences (bytes / str), or (bases, offsets): the reads the records' `read` fields index"""
        bases, offsets = reads if isinstance(reads, tuple) else concat_sequences(reads)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._call("set_reads", bases.ctypes.data if bases.size else None, offsets.ctypes.data, len(offsets) - 1)

    def add_records(self, recs):
        """FILL_RECORD_DTYPE records (any structured array with its first eight fields), behind those added so far"""
        if recs.dtype != FILL_RECORD_DTYPE:
            r = np.zeros(len(recs), dtype=FILL_RECORD_DTYPE)
            for f in FILL_RECORD_DTYPE.names[:8]:
                r[f] = recs[f]
            recs = r
        recs = np.ascontiguousarray(recs)
        self._call("add_records", recs.ctypes.data if len(recs) else None, len(recs))

    def add_hits(self, hits, first_read=0):
        """what Mapper.map (second_alignment) returned for reads first_read, first_read + 1, ...: MAP_HIT_DTYPE[n, 2]"""
        hits = np.ascontiguousarray(np.asarray(hits, dtype=MAP_HIT_DTYPE))
        if hits.ndim != 2 or hits.shape[1] != 2:
            raise ValueError("two hits per read")
        n = len(hits)
        self._call("add_hits", hits.ctypes.data if n else None, n, first_read)

    def build(self):
        self._call("build")

    def gap_stats(self):
        """-> SUPER_GAPSTAT_DTYPE per contig pair with a record, ascending by (contig_lo, contig_hi)"""
        n = C.c_uint64()
        self._call("gap_stats", None, 0, C.byref(n))
        out = np.zeros(max(n.value, 1), dtype=SUPER_GAPSTAT_DTYPE)
        self._call("gap_stats", out.ctypes.data, len(out), C.byref(n))
        return out[:n.value]

    def resolve(self):
        """-> the summary as a dict; a slice outside its read raises DbgkError (ERR_ARG) whose `bad` names record, read and contigs"""
        s = SuperSummary()
        rc = self._call("resolve", C.byref(s), ok=(0, ERR_ARG))
        if rc:
            e = DbgkError(rc, "dbgk_super_resolve")
            e.bad = {f: getattr(s, f) for f in ("bad_record", "bad_read", "bad_left", "bad_right")}
            raise e
        return {f: getattr(s, f) for f, _ in SuperSummary._fields_}

    def layout(self):
        """-> scaf_first[super-contigs + 1], LINK_ITEM_DTYPE items, SUPER_JUNCTION_DTYPE junctions, repeat contigs: in output order"""
        s = self.resolve()
        scaf_first = np.zeros(s["scaffolds"] + 1, dtype=np.uint64)
        items = np.zeros(max(s["items"], 1), dtype=LINK_ITEM_DTYPE)
        junctions = np.zeros(max(s["junctions"], 1), dtype=SUPER_JUNCTION_DTYPE)
        repeats = np.zeros(max(s["repeat_nodes"], 1), dtype=np.int32)
        self._call("layout", scaf_first.ctypes.data, items.ctypes.data, junctions.ctypes.data, repeats.ctypes.data)
        return scaf_first, items[:s["items"]], junctions[:s["junctions"]], repeats[:s["repeat_nodes"]]

    def slices(self):
        """-> SUPER_SLICE_DTYPE per slice (those of gap 1 first, per gap as sorted by length), and the bytes of the written ones"""
        s = self.resolve()
        n = C.c_uint64()
        out = np.zeros(max(s["slices"], 1), dtype=SUPER_SLICE_DTYPE)
        self._call("slices", out.ctypes.data, len(out), C.byref(n))
        data = np.zeros(max(s["slice_bytes"], 1), dtype=np.uint8)
        self._call("slice_bytes", data.ctypes.data, len(data), C.byref(n))
        return out[:s["slices"]], data[:s["slice_bytes"]]

    def timing(self):
        s = SuperTiming()
        self._call("batch_stats", C.byref(s))
        return {f: getattr(s, f) for f, _ in SuperTiming._fields_}


class ContigBuilder(_Handle):
    """The contig read-out on the GPU (CONTIG section of include/dbgk.h).  set_table(array, nul_flag, del_flag, klink) takes the
    host-layout table after simplification: NODE_DTYPE array[size], the two flag arrays of size // 8 + 1 bytes (bit 128 >> (i % 8)
    of byte i // 8), the 2-byte link records (bit 8 = linear).  read_out() -> bases, depths, offsets, records, summary: contigs in
    the order the reference's scan finds them.  wide=True: k up to 63 on a table of NODE32_DTYPE nodes (128-bit keys; parity
    unpinned above k = 32), everything else the same."""
    _destroy = "dbgk_contig_destroy"

    def __init__(self, k, kmer_freq_cutoff=2, contig_len_cutoff=125, device=0, wide=False):
        self.wide = bool(wide)
        self._h = C.c_void_p()
        self._keep = None
        create = "dbgk_wide_contig_create" if self.wide else "dbgk_contig_create"
        _chk(getattr(lib(), create)(C.byref(ContigParams(k, kmer_freq_cutoff, contig_len_cutoff, 0)), device, C.byref(self._h)), create)

    def set_table(self, array, nul_flag, del_flag, klink):
        array = np.ascontiguousarray(array, dtype=NODE32_DTYPE if self.wide else NODE_DTYPE)
        size = len(array)
        nul_flag = np.ascontiguousarray(nul_flag, dtype=np.uint8)
        del_flag = np.ascontiguousarray(del_flag, dtype=np.uint8)
        klink = np.ascontiguousarray(klink, dtype=np.uint16)
        if len(nul_flag) != size // 8 + 1 or len(del_flag) != size // 8 + 1 or len(klink) != size:
            raise ValueError("flag arrays of size // 8 + 1 bytes and one link record per slot")
        self._keep = (array, nul_flag, del_flag, klink)   # the host walker reads them during read_out
        set_table = "dbgk_wide_contig_set_table" if self.wide else "dbgk_contig_set_table"
        _chk(getattr(lib(), set_table)(self._h, size, array.ctypes.data, nul_flag.ctypes.data, del_flag.ctypes.data, klink.ctypes.data), set_table)

    def read_out(self):
        """-> bases (uint8), depths (uint8), offsets (uint64, contigs + 1), records (CONTIG_RECORD_DTYPE), summary (dict)"""
        s = ContigSummary()
        _chk(lib().dbgk_contig_read_out(self._h, C.byref(s)), "dbgk_contig_read_out")
        offsets = np.zeros(s.contigs + 1, dtype=np.uint64)
        records = np.zeros(max(s.contigs, 1), dtype=CONTIG_RECORD_DTYPE)
        bases = np.zeros(max(s.bytes, 1), dtype=np.uint8)
        depths = np.zeros(max(s.bytes, 1), dtype=np.uint8)
        _chk(lib().dbgk_contig_results(self._h, offsets.ctypes.data, records.ctypes.data, bases.ctypes.data, depths.ctypes.data),
             "dbgk_contig_results")
        return bases[:s.bytes], depths[:s.bytes], offsets, records[:s.contigs], self.summary()

    def summary(self):
        s = ContigSummary()
        _chk(lib().dbgk_contig_summary_get(self._h, C.byref(s)), "dbgk_contig_summary_get")
        return {f: getattr(s, f) for f, _ in ContigSummary._fields_ if f != "reserved"}

    def timing(self):
        s = ContigTiming()
        _chk(lib().dbgk_contig_timing_get(self._h, C.byref(s)), "dbgk_contig_timing_get")
        return {f: getattr(s, f) for f, _ in ContigTiming._fields_}

    def _trace_results(self, s):
        rows = np.zeros(max(s.rows, 1), dtype=TRACE_ROW_DTYPE)
        first = np.zeros(s.rows + 1, dtype=np.uint64)
        nodes = np.zeros(max(s.nodes, 1), dtype=np.uint32)
        bases = np.zeros(max(s.nodes, 1), dtype=np.uint8)
        _chk(lib().dbgk_simplify_trace_results(self._h, rows.ctypes.data, first.ctypes.data, nodes.ctypes.data, bases.ctypes.data),
             "dbgk_simplify_trace_results")
        return rows[:s.rows], first, nodes[:s.nodes], bases[:s.nodes], {f: getattr(s, f) for f, _ in TraceSummary._fields_}

    def trace(self, slots, directs, len_cutoff):
        """get_linear_path(slots[i], directs[i], len_cutoff) for every i (SIMPLIFY section of include/dbgk.h) -> rows (TRACE_ROW_DTYPE),
        node offsets (uint64, rows + 1), nodes (uint32 slots), bases (uint8 codes 0..3 = ACGT), summary (dict)"""
        req = np.zeros(len(slots), dtype=TRACE_REQUEST_DTYPE)
        req["slot"], req["direct"] = slots, directs
        s = TraceSummary()
        _chk(lib().dbgk_simplify_trace(self._h, req.ctypes.data if len(req) else None, len(req), len_cutoff, C.byref(s)), "dbgk_simplify_trace")
        return self._trace_results(s)

    def trace_branches(self, slots, len_cutoff):
        """8 rows per branching slot, row 8 i + 4 side + j (side 0 right, 1 left; base j) -> as trace()"""
        slots = np.ascontiguousarray(slots, dtype=np.uint64)
        s = TraceSummary()
        _chk(lib().dbgk_simplify_trace_branches(self._h, slots.ctypes.data if len(slots) else None, len(slots), len_cutoff, C.byref(s)),
             "dbgk_simplify_trace_branches")
        return self._trace_results(s)

    def update(self, slots):
        """the arrays given to set_table were changed in place at these slots: carry link words, link records and delete bits over"""
        slots = np.ascontiguousarray(slots, dtype=np.uint64)
        _chk(lib().dbgk_simplify_update(self._h, slots.ctypes.data if len(slots) else None, len(slots)), "dbgk_simplify_update")

    def simplify_timing(self):
        s = SimplifyTiming()
        _chk(lib().dbgk_simplify_timing_get(self._h, C.byref(s)), "dbgk_simplify_timing_get")
        return {f: getattr(s, f) for f, _ in SimplifyTiming._fields_ if f != "reserved"}

    def align(self, pairs):
        """global_aligning(a, b) for every (a, b) of pairs (str or bytes over ACGT; SIMPLIFY section of include/dbgk.h) -> rows
        (ALIGN_ROW_DTYPE), the aligned first strings and the aligned second strings (lists of bytes; b"" for a pair that is
        ALIGN_TOO_LONG), summary (dict).  Needs no table."""
        seqs = [x.encode() if isinstance(x, str) else bytes(x) for pair in pairs for x in pair]
        offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(x) for x in seqs], dtype=np.uint64)
        blob = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)
        n = len(seqs) // 2
        s = AlignSummary()
        _chk(lib().dbgk_align_pairs(self._h, blob.ctypes.data if n else None, offsets.ctypes.data if n else None, n, C.byref(s)), "dbgk_align_pairs")
        rows = np.zeros(max(n, 1), dtype=ALIGN_ROW_DTYPE)
        first = np.zeros(n + 1, dtype=np.uint64)
        a_i = np.zeros(max(s.aligned_bytes, 1), dtype=np.uint8)
        a_j = np.zeros(max(s.aligned_bytes, 1), dtype=np.uint8)
        _chk(lib().dbgk_align_results(self._h, rows.ctypes.data, first.ctypes.data, a_i.ctypes.data, a_j.ctypes.data), "dbgk_align_results")
        cut = [int(v) for v in first]
        return (rows[:n], [a_i[cut[p]:cut[p + 1]].tobytes() for p in range(n)], [a_j[cut[p]:cut[p + 1]].tobytes() for p in range(n)],
                {f: getattr(s, f) for f, _ in AlignSummary._fields_ if f != "reserved"})

    def align_timing(self):
        s = AlignTiming()
        _chk(lib().dbgk_align_timing_get(self._h, C.byref(s)), "dbgk_align_timing_get")
        return {f: getattr(s, f) for f, _ in AlignTiming._fields_ if f != "reserved"}
