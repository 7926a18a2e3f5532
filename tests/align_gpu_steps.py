"""GPU steps of tests/test_align_gpu.py, each run in a child process of its own under a time limit:
    python tests/align_gpu_steps.py pairs | arguments  bare | table | wide
capi.ContigBuilder.align over every pair of tests/golden/align_cases/pairs.npz, byte for byte against what the reference's
global_aligning() returned: on a handle without a table (bare), on one with a table set (table), on a handle for 128-bit keys (wide).
Prints one JSON line of findings; exits non-zero on a mismatch."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
from contig_gpu_steps import build_table, rand_seq  # noqa: E402
from test_align_cpu import load_pairs  # noqa: E402


def builder(mode):
    from dbg_assembly_amd import capi
    g = capi.ContigBuilder(21, wide=mode == "wide")
    if mode == "table":
        t = build_table([(rand_seq(random.Random(5), 80), 5)], 21, 211)
        R.first_pass(t, R.Options())
        g.set_table(*t.arrays())
    return g


def compare(got, pairs, what):
    from dbg_assembly_amd import capi
    rows, a_i, a_j, summ = got
    assert len(rows) == len(a_i) == len(a_j) == len(pairs) == summ["pairs"], (what, summ)
    for n, (si, sj, ai, aj, score, fits) in enumerate(pairs):
        r = rows[n]
        g = tuple(int(r[f]) for f in ("len_i", "len_j", "score", "aligned_len", "diffs", "status")) + (tuple(int(v) for v in r["pad"]),)
        if fits:
            want = (len(si), len(sj), score, len(ai), R.count_differences(ai.decode(), aj.decode()), capi.ALIGN_DONE, (0, 0, 0))
        else:
            want = (len(si), len(sj), 0, 0, 0, capi.ALIGN_TOO_LONG, (0, 0, 0))
        assert g == want, (what, n, g, want)
        assert (a_i[n], a_j[n]) == (ai, aj), (what, n, si, sj)
    assert summ["aligned"] == sum(1 for p in pairs if p[5]) and summ["too_long"] == sum(1 for p in pairs if not p[5]), (what, summ)
    assert summ["aligned_bytes"] == sum(len(p[2]) for p in pairs), (what, summ)


def step_pairs(mode):
    pairs = load_pairs()
    strings = [(p[0], p[1]) for p in pairs]
    out = {"pairs": len(pairs)}
    with builder(mode) as g:
        one = g.align(strings)
        compare(one, pairs, "one batch")
        out["batches"] = one[3]["batches"]
        os.environ["DBGK_TEST_HOOKS"] = "align_batch=3"
        three = g.align(strings)
        del os.environ["DBGK_TEST_HOOKS"]
        compare(three, pairs, "batches of 3")
        assert np.array_equal(one[0], three[0]) and one[1] == three[1] and one[2] == three[2], "batches of 3 differ from one batch"
        out["batches_of_3"] = three[3]["batches"]
        # a batch is a kernel launch: three pairs that are all above the bound make none
        out["launches_for_3"] = sum(1 for n in range(0, len(pairs), 3) if any(p[5] for p in pairs[n:n + 3]))
        # 1, 63, 64 and 65 pairs: fewer pairs than workgroups, and a grid that is no multiple of anything
        for n in (1, 63, 64, 65):
            compare(g.align(strings[:n]), pairs[:n], n)
        none = g.align([])
        assert len(none[0]) == 0 and none[3]["batches"] == 0 and none[3]["pairs"] == 0
        tm = g.align_timing()
        out["timing_pairs"], out["cells"], out["bytes_back"] = tm["pairs"], tm["cells"], tm["bytes_back"]
        fits = [1 if p[5] else 0 for p in pairs]
        assert tm["pairs"] == 2 * sum(fits) + sum(sum(fits[:n]) for n in (1, 63, 64, 65)), tm
        assert tm["batches"] == out["batches"] + out["batches_of_3"] + 4 and tm["ms_align"] > 0 and tm["bytes_up"] > 0
    return out


def step_arguments(mode):
    """all before device work: the handle's timing does not move"""
    from dbg_assembly_amd import capi
    checked = 0
    with builder(mode) as g:
        try:
            capi._chk(capi.lib().dbgk_align_results(g._h, None, None, None, None), "dbgk_align_results")
        except capi.DbgkError as e:
            assert e.status == capi.ERR_STATE, e.status
            checked += 1
        else:
            raise AssertionError("results before any align call were accepted")
        for bad in ([("", "ACGT")], [("ACGT", "")], [("ACGT", "ACNT")], [("acgt", "ACGT")], [("ACGT", "AC-T")], [("AC", "GT"), ("A", "")]):
            try:
                g.align(bad)
            except capi.DbgkError as e:
                assert e.status == capi.ERR_ARG, e.status
                checked += 1
            else:
                raise AssertionError("a bad pair was accepted: %r" % (bad,))
        # decreasing offsets
        seqs = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
        off = np.array([0, 4, 2], dtype=np.uint64)
        s = capi.AlignSummary()
        assert capi.lib().dbgk_align_pairs(g._h, seqs.ctypes.data, off.ctypes.data, 1, C.byref(s)) == capi.ERR_ARG
        assert capi.lib().dbgk_align_pairs(g._h, None, None, 1, C.byref(s)) == capi.ERR_ARG
        checked += 2
        tm = g.align_timing()
        assert tm["batches"] == 0 and tm["pairs"] == 0 and tm["bytes_up"] == 0, tm
        rows, a_i, a_j, summ = g.align([("ACGT", "ACT")])          # the handle still works
        want = R.global_align("ACGT", "ACT")
        assert (a_i[0].decode(), a_j[0].decode()) == want and int(rows[0]["aligned_len"]) == len(want[0]) and summ["batches"] == 1, (rows, a_i, a_j)
    return {"argument_checks": checked}


if __name__ == "__main__":
    res = {"pairs": step_pairs, "arguments": step_arguments}[sys.argv[1]](sys.argv[2])
    print(json.dumps(res))
