"""CPU restatement of the corrector's output stage (csrc/dbgk_emit.h, CorrRule) in numpy: the length rule of the command line
(host/correct_error_reads.cpp:155), the compact offsets, the gather and the counters of <file>.correct.stat.  Pinned to the
reference by tests/test_corr_compact_cpu.py: applied to the output of tests/correct_restatement.py it gives the sequence
lines and the stat numbers of every golden the real reference wrote."""
import numpy as np

REC_DTYPE = np.dtype([("one_base", "<u4"), ("tree", "<u4"), ("left_trim", "<u4"), ("right_trim", "<u4"),
                      ("node_limit_hits", "<u4"), ("deleted", "u1"), ("path", "u1"), ("pad", "u1", (2,))])   # dbgk_corr_rec
COUNTERS = ("reads", "result_reads", "result_bases", "trimmed_reads", "trimmed_bases", "deleted_reads", "one_base", "tree",
            "node_limit_hits", "by_classify", "by_correct", "by_overflow")


def out_lengths(offsets, rec):
    """deleted ? 0 : L - left_trim - right_trim; a record that trims more than its read holds (the kernels write none for a
    read they keep: such a read has L - lt - rt < 0 <= -r and is deleted) gives 0"""
    L = np.diff(np.asarray(offsets, dtype=np.uint64)).astype(np.int64)
    cut = rec["left_trim"].astype(np.int64) + rec["right_trim"].astype(np.int64)
    return np.where((rec["deleted"] != 0) | (cut >= L), 0, L - cut).astype(np.uint64)


def compact(out, offsets, rec):
    """-> (compact bases uint8, compact offsets uint64[n + 1], counters): read i contributes
    out[offsets[i] + left_trim : offsets[i] + left_trim + length], reads of length 0 keep their place"""
    out = np.asarray(out, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    lens = out_lengths(offsets, rec)
    coff = np.zeros(n + 1, dtype=np.uint64)
    coff[1:] = np.cumsum(lens)
    total = int(coff[n])
    # the gather: output byte j belongs to read i = the last one with coff[i] <= j among those that hold bytes
    owner = np.repeat(np.arange(n, dtype=np.int64), lens.astype(np.int64))
    src = offsets[:-1].astype(np.int64)[owner] + rec["left_trim"].astype(np.int64)[owner] + (np.arange(total, dtype=np.int64) - coff[:-1].astype(np.int64)[owner])
    bases = out[src] if total else np.zeros(0, dtype=np.uint8)
    kept = rec["deleted"] == 0
    trimmed = kept & ((rec["left_trim"] > 0) | (rec["right_trim"] > 0))
    cnt = {"reads": n, "result_reads": int(kept.sum()), "result_bases": int(lens[kept].sum()), "trimmed_reads": int(trimmed.sum()),
           "trimmed_bases": int(rec["left_trim"][trimmed].astype(np.int64).sum() + rec["right_trim"][trimmed].astype(np.int64).sum()),
           "deleted_reads": int((~kept).sum()), "one_base": int(rec["one_base"][kept].astype(np.int64).sum()),
           "tree": int(rec["tree"][kept].astype(np.int64).sum()), "node_limit_hits": int(rec["node_limit_hits"].astype(np.int64).sum()),
           "by_classify": int((rec["path"] == 0).sum()), "by_correct": int((rec["path"] == 1).sum()), "by_overflow": int((rec["path"] == 2).sum())}
    return bases, coff, cnt


def sequence_lines(fa):
    """the sequence lines of a decompressed .correct.fa (every second line; a deleted read's is empty)"""
    lines = fa.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    return lines[1:-1:2]


def as_lines(bases, coff):
    b = np.asarray(bases, dtype=np.uint8).tobytes()
    return [b[int(coff[i]):int(coff[i + 1])] for i in range(len(coff) - 1)]


def stat_numbers(text):
    """the integer lines of a .correct.stat as {name: value}"""
    out = {}
    for line in text.splitlines():
        t = line.split()
        if len(t) == 2 and t[1].isdigit():
            out[t[0]] = int(t[1])
    return out


def stat_of(cnt, raw_bases):
    """the same numbers from the counters of a single-batch file"""
    return {"num_raw_reads": cnt["reads"], "num_raw_bases": raw_bases, "num_result_reads": cnt["result_reads"],
            "num_result_bases": cnt["result_bases"], "num_trimmed_reads": cnt["trimmed_reads"], "num_trimmed_bases": cnt["trimmed_bases"],
            "num_deleted_reads": cnt["deleted_reads"], "num_corrected_bases_by_Fast_method": cnt["one_base"],
            "num_corrected_bases_by_BBtree_method": cnt["tree"], "num_corrected_bases_by_two_methods": cnt["one_base"] + cnt["tree"]}


def records_of(rows):
    """(one_base, tree, deleted, left_trim, right_trim, node_limit_hits[, path]) per read -> REC_DTYPE"""
    rec = np.zeros(len(rows), dtype=REC_DTYPE)
    for i, r in enumerate(rows):
        rec[i]["one_base"], rec[i]["tree"], rec[i]["deleted"], rec[i]["left_trim"], rec[i]["right_trim"], rec[i]["node_limit_hits"] = r[:6]
        rec[i]["path"] = r[6] if len(r) > 6 else 0
    return rec
