"""CPU: link_scaffold -- the command line, the argument checks of the C ABI, the binding, and the Python restatement of the
program against every golden the real reference wrote (tests/golden/link_cases, both E. coli runs included)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import link_restatement as LR  # noqa: E402

BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLDEN, "link_cases")


def golden_cases():
    return LR.golden_cases(CASES)


def compare_outputs(case, got, want):
    """byte for byte; the tie case as a multiset of records with their scaffold ids blanked (std::sort promises no order there)"""
    assert sorted(got) == sorted(want)
    for f in sorted(want):
        if case["tie"] and f.endswith((".pos.tab", ".seq.fa")):
            assert LR.split_records(got[f]) == LR.split_records(want[f]), f
        else:
            assert got[f] == want[f], f


def test_cli_prints_the_reference_usage():
    want = open(os.path.join(GOLDEN, "link_usage.txt"), "rb").read()
    prog = os.path.join(BIN, "link_scaffold")
    r = subprocess.run([prog], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == want
    assert subprocess.run([prog, "-h"], capture_output=True, timeout=60).stdout == want
    assert subprocess.run([prog, "only_one_argument"], capture_output=True, timeout=60).stdout == want


def test_link_entry_points_validate_before_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p()
    good = dict(mate_pair=0, pair_num_cut=3, insert_size=400)
    for bad in (dict(mate_pair=2), dict(mate_pair=-1), dict(pair_num_cut=-1), dict(insert_size=0), dict(insert_size=-400)):
        p = capi.LinkParams(**dict(good, **bad))
        assert L.dbgk_link_create(ctypes.byref(p), 0, ctypes.byref(h)) == capi.ERR_ARG, bad
    p = capi.LinkParams(**good)
    assert L.dbgk_link_create(None, 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_link_create(ctypes.byref(p), -1, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_link_create(ctypes.byref(p), 0, None) == capi.ERR_ARG
    n = ctypes.c_uint64()
    buf = (ctypes.c_uint64 * 16)()
    assert L.dbgk_link_destroy(None) == capi.ERR_ARG
    assert L.dbgk_link_set_contigs(None, buf, 1) == capi.ERR_ARG
    assert L.dbgk_link_add_pairs(None, buf, 1) == capi.ERR_ARG
    assert L.dbgk_link_add_hits(None, buf, buf, 1) == capi.ERR_ARG
    assert L.dbgk_link_build(None) == capi.ERR_ARG
    assert L.dbgk_link_export(None, None, None, 0, ctypes.byref(n), None) == capi.ERR_ARG
    assert L.dbgk_link_resolve(None, None) == capi.ERR_ARG
    assert L.dbgk_link_snapshot(None, 0, None, None, None) == capi.ERR_ARG
    assert L.dbgk_link_layout(None, None, None, None) == capi.ERR_ARG
    assert L.dbgk_link_emit(None, None, buf, 0, None, 0, None, 0, ctypes.byref(n)) == capi.ERR_ARG
    assert L.dbgk_link_batch_stats(None, None) == capi.ERR_ARG


def test_binding_covers_the_link_section():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in ("create", "destroy", "set_contigs", "add_pairs", "add_hits", "build", "export", "resolve", "snapshot", "layout", "emit",
              "batch_stats"):
        assert "dbgk_link_" + n in names and hasattr(capi.lib(), "dbgk_link_" + n)
    assert capi.LINK_PAIR_DTYPE.itemsize == 32 and capi.LINK_ENTRY_DTYPE.itemsize == 16 and capi.LINK_ITEM_DTYPE.itemsize == 8
    assert capi.LINK_PAIR_DTYPE.fields["direct1"][1] == 24 and capi.LINK_ENTRY_DTYPE.fields["size"][1] == 8
    assert ctypes.sizeof(capi.LinkParams) == 12 and ctypes.sizeof(capi.LinkCounters) == 40 and ctypes.sizeof(capi.LinkSummary) == 48
    assert ctypes.sizeof(capi.LinkTiming) == 5 * 8 + 5 * 8
    assert [LR.PAIR_DTYPE.fields[f][1] for f in LR.PAIR_DTYPE.names[:8]] == [capi.LINK_PAIR_DTYPE.fields[f][1] for f in LR.PAIR_DTYPE.names[:8]]
    assert capi.lib().dbgk_abi_version() == 7
    assert hasattr(capi.Scaffolder, "__enter__") and hasattr(capi.Scaffolder, "add_hits")


def test_no_scaffolder_without_gpu(tmp_path):
    """no device: the binding raises and the program exits non-zero with a message, nothing falls back to the host"""
    from dbg_assembly_amd import capi
    if capi.lib().dbgk_device_count() > 0:
        return
    with pytest.raises(capi.DbgkError) as e:
        capi.Scaffolder()
    assert e.value.status == capi.ERR_HIP
    LR.unpack_inputs(CASES, next(c for c in golden_cases() if c["name"] == "pe_n1"), tmp_path / "c")
    r = subprocess.run([os.path.join(BIN, "link_scaffold"), "-o", "x", "contigs.fa", "pairs.lib"], cwd=tmp_path / "c", capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "dbgk_link_create failed" in r.stderr


def test_cli_refuses_contig_names_the_reference_cannot_index(tmp_path):
    (tmp_path / "c.fa").write_text(">ctg_1\nACGT\n>ctg_5\nACGT\n")
    (tmp_path / "p.lib").write_text("")
    r = subprocess.run([os.path.join(BIN, "link_scaffold"), "c.fa", "p.lib"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "its number must be 3" in r.stderr
    with pytest.raises(ValueError):
        LR.check_names(["ctg_1", "ctg_5"])


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_golden(case):
    want = LR.expected_outputs(CASES, case)
    got, res = LR.run_case(CASES, case)
    assert len(want) == (5 if "lengths" in case else 7)
    compare_outputs(case, got, want)
    if "counters" in case:
        assert res["counters"] == case["counters"]


def test_goldens_cover_what_they_are_meant_to():
    cases = {c["name"]: c for c in golden_cases()}
    assert sum(c["tie"] for c in cases.values()) == 1
    assert {LR.case_params(c).m for c in cases.values()} == {0, 1}
    assert {0, 1, 3} <= {LR.case_params(c).n for c in cases.values()} and any(LR.case_params(c).i % 2 for c in cases.values())
    e4, e8 = cases["ecoli_insert400"]["counters"], cases["ecoli_insert800"]["counters"]
    eff = lambda c: c["FR"] + c["RF"] + c["FF"] + c["RR"]  # noqa: E731
    assert (eff(e4), e4["interleave"], e4["repeat"], e4["scaffolds"]) == (6479, 37, 78, 131)
    assert (eff(e8), e8["interleave"], e8["repeat"], e8["scaffolds"]) == (769, 0, 8, 90)
    all_text = LR.expected_outputs(CASES, cases["pe_default"])["res_pe_default.insert400.scaffold.links.all"]
    assert "\t53,1023,-51150,-50" in all_text and ",4,-123,-30" in all_text     # the 1023 cap; a truncated negative average
    for name in ("pe_default", "mp_default"):
        err = LR.expected_outputs(CASES, cases[name])["stderr.txt"]
        assert "Wrong_link_num: 3\n" in err and "Removed interleave links num: 4\n" in err and "files number: 2\n" in err


def test_restatement_pieces():
    assert LR.reverse_complement("acgtnNRYx-ACGT") == "ACGTNNNNNnACGT"
    assert [LR.c_div(a, b) for a, b in ((-123, 4), (123, 4), (-1, 3), (-51150, 1023))] == [-30, 30, 0, -50]
    v = [(n % 7, n) for n in range(200)]
    LR.std_sort(v, LR.by_len)
    assert [x[0] for x in v] == sorted((n % 7 for n in range(200)), reverse=True)
    P = LR.Params(m=0, n=3, i=401)
    recs = np.zeros(4, dtype=LR.PAIR_DTYPE)
    recs["contig1"], recs["contig2"], recs["direct1"], recs["direct2"] = 0, 1, ord("F"), ord("R")
    recs["start1"] = 950                                     # gap = 401 - 50 - end2
    recs["end2"] = [551, 550, -50, -51]                      # -200 (dropped: -401 / 2 is -200), -199, 401, 402 (dropped)
    assert LR.orient(P, [1000, 1000], recs)[5].tolist() == [False, True, True, False]
