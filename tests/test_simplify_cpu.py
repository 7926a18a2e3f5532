"""CPU: the SIMPLIFY calls of the library without a GPU -- symbols, struct layouts, and the argument checks that come before any
device work and need no handle (a handle cannot be made without a device; the checks that need a table run in
tests/simplify_gpu_steps.py)."""
import ctypes as C
import os
import re

import numpy as np

from dbg_assembly_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dbgk_simplify_timing_get", "dbgk_simplify_trace", "dbgk_simplify_trace_branches", "dbgk_simplify_trace_results", "dbgk_simplify_update"]


def test_simplify_symbols_and_layouts():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "dbgk.h")).read()
    assert sorted(n for n, _, _ in capi.SYMBOLS if n.startswith("dbgk_simplify_")) == NAMES
    for n in NAMES:
        assert hasattr(L, n) and ("int %s(" % n) in header
    assert capi.TRACE_ROW_DTYPE.itemsize == 24 and capi.TRACE_REQUEST_DTYPE.itemsize == 16
    assert C.sizeof(capi.TraceSummary) == 32 and C.sizeof(capi.SimplifyTiming) == 64
    assert capi.TRACE_MAX_CUTOFF == int(re.search(r"#define\s+DBGK_TRACE_MAX_CUTOFF\s+(\d+)", header).group(1))
    assert all(hasattr(capi.ContigBuilder, m) for m in ("trace", "trace_branches", "update", "simplify_timing"))


def test_null_handle_is_an_argument_error_before_any_device_work():
    L = capi.lib()
    req = np.zeros(1, dtype=capi.TRACE_REQUEST_DTYPE)
    slots = np.zeros(1, dtype=np.uint64)
    s, t = capi.TraceSummary(), capi.SimplifyTiming()
    assert L.dbgk_simplify_trace(None, req.ctypes.data, 1, 100, C.byref(s)) == capi.ERR_ARG
    assert L.dbgk_simplify_trace_branches(None, slots.ctypes.data, 1, 100, C.byref(s)) == capi.ERR_ARG
    assert L.dbgk_simplify_trace_results(None, None, None, None, None) == capi.ERR_ARG
    assert L.dbgk_simplify_update(None, slots.ctypes.data, 1) == capi.ERR_ARG
    assert L.dbgk_simplify_timing_get(None, C.byref(t)) == capi.ERR_ARG


def test_no_builder_without_a_gpu():
    """no host fall-back: without a device there is no handle to trace on"""
    if capi.lib().dbgk_device_count() > 0:
        return
    try:
        capi.ContigBuilder(21)
    except capi.DbgkError as e:
        assert e.status == capi.ERR_HIP
    else:
        raise AssertionError("a contig handle was made without a GPU")


# ---- the validation rule, restated (tests/simplify_restatement.py): no GPU ----
import sys  # noqa: E402

import pytest  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
import simplify_restatement as S  # noqa: E402
from test_contig_cpu import golden_cases, load_case  # noqa: E402


@pytest.mark.parametrize("name", golden_cases())
def test_passes_over_validated_traces_reproduce_the_reference(name):
    """the passes' three files from walks that are traces of the pass's snapshot wherever the three conditions hold; every trace used
    is asserted to be the live walk (simplify_restatement.Pass.walk)"""
    c = load_case(name)
    o = R.Options.from_args(c["args"])
    files, counts, err = S.run_passes(R.Table.from_case(c), o)
    assert sorted(files) == sorted(s for s in c["files"] if s in ("tip.fa", "lowedge.fa", "bubble.fa"))
    for s in files:
        assert files[s] == c["files"][s], (name, s)
    plain, none, err2 = S.run_passes(R.Table.from_case(c), o, traced=False)
    assert plain == files and err == err2 and all(v[1] == 0 and v[2] == 0 for v in none.values())
    if name == "e_no_passes":
        assert counts == {}
    if name == "b_tips":
        assert counts["tips"][2] > 0          # the one golden in which a removal reaches into a later walk


NEW_CASES = os.path.join(ROOT, "tests", "golden", "simplify_cases")
NEW_NAMES = ["a_two_tips_one_node", "b_facing_tips", "c_last_on_earlier_tip", "d_lowedges_one_end", "e_bubble_after_bubble", "f_tip_and_bubble"]


def test_the_six_ordering_cases_are_there():
    assert sorted(f[:-4] for f in os.listdir(NEW_CASES) if f.endswith(".npz")) == NEW_NAMES


@pytest.mark.parametrize("name", NEW_NAMES)
def test_ordering_cases_reproduce_the_reference_and_fall_back(name):
    """tests/golden/simplify_cases (the real reference at -t 1): the restated rule writes the reference's files, equals the plain
    passes, gives the counts recorded when the case was made, and sends at least one walk back to the host"""
    c = R.load_case(os.path.join(NEW_CASES, name + ".npz"))
    o = R.Options.from_args(c["args"])
    files, counts, err = S.run_passes(R.Table.from_case(c), o)
    assert sorted(files) == ["bubble.fa", "lowedge.fa", "tip.fa"]
    for s in files:
        assert files[s] == c["files"][s], (name, s)
    stage_files, _, _ = R.run_stage(R.Table.from_case(c), o)
    assert all(stage_files[s] == c["files"][s] for s in c["files"])
    plain, _, err2 = S.run_passes(R.Table.from_case(c), o, traced=False)
    assert plain == files and err == err2
    assert {p: list(v) for p, v in counts.items()} == c["shows"]["counts"]
    assert sum(v[2] for v in counts.values()) > 0 and all(v[1] + v[2] <= v[0] for v in counts.values())


def test_rule_holds_where_removals_crowd_each_other():
    """reads with many errors at -D 0: tips and bubbles by the hundred on a small table, so that removals change what later walks
    touch; the files equal those of the plain passes and the rule sends a share of the walks back to the host"""
    import random
    from contig_gpu_steps import build_table
    rng = random.Random(17)
    genome = "".join(rng.choices("ACGT", k=3000))
    reads = []
    for _ in range(600):
        p = rng.randrange(len(genome) - 100)
        r = list(genome[p:p + 100])
        for q in range(100):
            if rng.random() < 0.01:
                r[q] = rng.choice([b for b in "ACGT" if b != r[q]])
        reads.append(("".join(r), 1))
    o = R.Options(D=0, I=30, C=30, U=30)
    a, b = build_table(reads, 21, 40009), build_table(reads, 21, 40009)
    files, counts, err = S.run_passes(a, o)
    plain, _, err2 = S.run_passes(b, o, traced=False)
    assert files == plain and err == err2
    assert a.deleted == b.deleted and a.l_link == b.l_link and a.r_link == b.r_link and a.linear == b.linear
    print(counts)
    assert all(v[1] > 50 for v in counts.values()) and sum(v[2] for v in counts.values()) > 20
