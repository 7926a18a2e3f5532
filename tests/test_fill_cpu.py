"""CPU: link_contig -- the command line, the argument checks of the C ABI, the binding, and the Python restatement of the program
against every golden the real reference wrote (tests/golden/fill_cases)."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fill_restatement as FR  # noqa: E402
import link_restatement as LR  # noqa: E402

BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLDEN, "fill_cases")


def golden_cases():
    return FR.golden_cases(CASES)


def test_cli_prints_the_reference_usage():
    want = open(os.path.join(GOLDEN, "fill_usage.txt"), "rb").read()
    prog = os.path.join(BIN, "link_contig")
    r = subprocess.run([prog], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == want
    assert subprocess.run([prog, "-h"], capture_output=True, timeout=60).stdout == want
    assert subprocess.run([prog, "only_one_argument"], capture_output=True, timeout=60).stdout == want
    # (the usage shows the value -n was given, as the reference's does)
    assert subprocess.run([prog, "-n", "5", "one"], capture_output=True, timeout=60).stdout == want.replace(b"default=3", b"default=5")


def test_fill_entry_points_validate_before_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p()
    good = capi.FillParams(3, (ctypes.c_int32 * 3)(0, 0, 0))
    assert L.dbgk_fill_create(ctypes.byref(capi.FillParams(-1, (ctypes.c_int32 * 3)(0, 0, 0))), 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_fill_create(ctypes.byref(capi.FillParams(3, (ctypes.c_int32 * 3)(0, 1, 0))), 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_fill_create(None, 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_fill_create(ctypes.byref(good), -1, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_fill_create(ctypes.byref(good), 0, None) == capi.ERR_ARG
    n = ctypes.c_uint64()
    buf = (ctypes.c_uint64 * 16)()
    assert L.dbgk_fill_destroy(None) == capi.ERR_ARG
    assert L.dbgk_fill_set_contigs(None, buf, 1) == capi.ERR_ARG
    assert L.dbgk_fill_set_reads(None, buf, buf, 1) == capi.ERR_ARG
    assert L.dbgk_fill_add_records(None, buf, 1) == capi.ERR_ARG
    assert L.dbgk_fill_add_hits(None, buf, 1, 0) == capi.ERR_ARG
    assert L.dbgk_fill_build(None) == capi.ERR_ARG
    assert L.dbgk_fill_export(None, None, None, 0, ctypes.byref(n), None) == capi.ERR_ARG
    assert L.dbgk_fill_gap_stats(None, None, 0, ctypes.byref(n)) == capi.ERR_ARG
    assert L.dbgk_fill_resolve(None, None) == capi.ERR_ARG
    assert L.dbgk_fill_snapshot(None, 0, None, None, None) == capi.ERR_ARG
    assert L.dbgk_fill_layout(None, None, None, None, None, None) == capi.ERR_ARG
    assert L.dbgk_fill_emit(None, None, buf, 0, None, 0, None, 0, ctypes.byref(n)) == capi.ERR_ARG
    assert L.dbgk_fill_batch_stats(None, None) == capi.ERR_ARG


def test_binding_covers_the_fill_section():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in ("create", "destroy", "set_contigs", "set_reads", "add_records", "add_hits", "build", "export", "gap_stats", "resolve",
              "snapshot", "layout", "emit", "batch_stats"):
        assert "dbgk_fill_" + n in names and hasattr(capi.lib(), "dbgk_fill_" + n)
    assert capi.FILL_RECORD_DTYPE.itemsize == 32 and capi.FILL_RECORD_DTYPE.fields["direct1"][1] == 24
    assert capi.FILL_GAPSTAT_DTYPE.itemsize == 24 and capi.FILL_ITEM_DTYPE.itemsize == 24 and capi.FILL_GAP_DTYPE.itemsize == 24
    assert capi.FILL_ITEM_DTYPE.fields["cons_off"][1] == 16
    assert ctypes.sizeof(capi.FillParams) == 16 and ctypes.sizeof(capi.FillSummary) == 72 and ctypes.sizeof(capi.FillTiming) == 96
    assert [FR.REC_DTYPE.fields[f][1] for f in FR.REC_DTYPE.names[:8]] == [capi.FILL_RECORD_DTYPE.fields[f][1] for f in FR.REC_DTYPE.names[:8]]
    assert capi.lib().dbgk_abi_version() == 7
    for m in ("set_contigs", "set_reads", "add_records", "add_hits", "build", "resolve", "gap_stats", "layout", "emit", "timing", "__enter__"):
        assert hasattr(capi.GapFiller, m), m
    assert list(inspect.signature(capi.GapFiller.__init__).parameters) == ["self", "pair_num_cut", "device"]
    assert list(inspect.signature(capi.GapFiller.add_hits).parameters) == ["self", "hits", "first_read"]
    assert capi.float9(1.0) == "1" and capi.float9(np.float32(5) / np.float32(6)) == "0.833333313"


def test_no_gap_filler_without_gpu(tmp_path):
    """no device: the binding raises and the program exits non-zero with a message, nothing falls back to the host"""
    from dbg_assembly_amd import capi
    if capi.lib().dbgk_device_count() > 0:
        return
    with pytest.raises(capi.DbgkError) as e:
        capi.GapFiller()
    assert e.value.status == capi.ERR_HIP
    case = next(c for c in golden_cases() if c["name"] == "n1")
    LR.unpack_inputs(CASES, case, tmp_path / "c")
    r = subprocess.run([os.path.join(BIN, "link_contig"), "-o", "x", case["contigs"], case["lib"]], cwd=tmp_path / "c", capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "dbgk_fill_create failed" in r.stderr


def test_cli_refuses_contig_names_the_reference_cannot_index(tmp_path):
    (tmp_path / "c.fa").write_text(">ctg_1\nACGT\n>ctg_5\nACGT\n")
    (tmp_path / "p.lib").write_text("")
    r = subprocess.run([os.path.join(BIN, "link_contig"), "c.fa", "p.lib"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "its number must be 3" in r.stderr


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_golden(case):
    want = LR.expected_outputs(CASES, case)
    got, _ = FR.run_case(CASES, case)
    assert len(want) == 7
    FR.compare_outputs(case, got, want)


def test_goldens_cover_what_they_are_meant_to():
    cases = {c["name"]: c for c in golden_cases()}
    assert {FR.case_params(c).n for c in cases.values()} == {1, 2, 3, 5} and sum(c["tie"] for c in cases.values()) == 1
    for name, case in cases.items():
        assert all(not n.endswith((".cpp", ".h", ".py", ".pl", ".sh")) and "Makefile" not in n for n in LR.case_files(CASES, case))
    _, res = FR.run_case(CASES, cases["n_default"])
    st = res["stats"]
    assert st[(5, 6)][:3] == (10, 3, 6)                 # a mode tie goes to the smaller gap
    assert st[(14, 15)][:3] == (9, 6, 7)                # conflicting and wrong-direction records are pooled
    assert st[(28, 29)][:3] == (3, 1040, 1070)          # the statistics are not capped at 1023 ...
    text = LR.expected_outputs(CASES, cases["n_default"])
    assert "\t59,1023,3069,3" in text["res_n_default.contig_R.links.all"]        # ... the link is
    assert "Wrong_link_num: 2\n" in text["stderr.txt"] and text["res_n_default.contig_R.repeat.seq.fa"]
    seq = text["res_n_default.contig_R.seq.fa"]
    assert "GGATGAC" in seq and "ACgTN" in seq and "ANNA" in seq
    gaps = [it for items in res["layout"] for it in items if it[0] == "gap"]
    assert any(g[1] > 0 for g in gaps) and any(g[1] == 0 for g in gaps) and any(g[1] < -14 for g in gaps)
    assert any(g[1] > 0 and float(g[6]) < 1 for g in gaps) and any(g[1] > 0 and float(g[6]) == 1 for g in gaps)
    _, tie = FR.run_case(CASES, cases["n2_tie"])
    lengths = [sum(FR.item_len(it) for it in items) for items in tie["layout"]]
    assert len(set(lengths)) < len(lengths)


def test_restatement_pieces():
    assert FR.consensus(["AC", "CC", "AT", "CG"])[:2] == ("AC", [2, 2])       # a tie goes to the smaller byte
    assert FR.float9(FR.consensus(["AAAAAA", "AAAAAC", "AAAAAA"])[2]) == "0.944444418"
    recs = np.zeros(5, dtype=FR.REC_DTYPE)
    recs["contig1"], recs["contig2"] = [0, 1, 0, 0, 1], [1, 0, 1, 1, 0]
    recs["align1_end"], recs["align2_start"] = 10, [21, 21, 15, 15, 40]
    m = FR.gap_stats(recs)[(0, 1)]
    assert m[:4] == (4, 2, 5, (6 * 2 + 25) // 5) and m[4].tolist() == [2, 3]
