"""CPU: correct_error_reads -- the command line, the argument checks of the C ABI, the binding, and the Python
restatement of correct_one_read against every golden the real reference wrote (tests/golden/correct_*)."""
import ctypes
import gzip
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import correct_restatement as CR  # noqa: E402

EXE = os.path.join(ROOT, "dbg_assembly_amd", "bin", "correct_error_reads")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_cases():
    out = []
    for d in sorted(os.listdir(GOLDEN)):
        if d.startswith("correct_") and d != "correct_edges" and os.path.isdir(os.path.join(GOLDEN, d)):   # test_correct_edges_cpu.py
            for c in json.load(open(os.path.join(GOLDEN, d, "cases.json"))):
                out.append((d, c))
    return out


def expected_fa(d, case):
    """the reference's .correct.fa of a golden case, decompressed"""
    return gzip.open(os.path.join(GOLDEN, d, case["name"] + ".correct.fa.gz"), "rb").read()


def params_of(case):
    a = case["args"]
    o = dict(zip(a[0::2], a[1::2]))
    return CR.Params(k=int(o["-k"]), m=int(o.get("-m", 17)), c=int(o.get("-c", 2)), x=int(o.get("-x", 17)),
                     n=int(o.get("-n", 5000000)), r=int(o.get("-r", 75)))


def test_cli_prints_the_reference_usage():
    want = open(os.path.join(GOLDEN, "correct_usage.txt"), "rb").read()
    r = subprocess.run([EXE], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == want
    r = subprocess.run([EXE, "-h"], capture_output=True, timeout=60)
    assert r.stdout == want


@pytest.mark.parametrize("opts,word", [(["-j", "1"], "-j 1"), (["-n", str(1 << 26)], "2^26")])
def test_cli_refuses_what_it_does_not_reproduce(tmp_path, opts, word):
    r = subprocess.run([EXE] + opts + [str(tmp_path / "t.cz"), str(tmp_path / "r.lib")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and word in r.stderr


def test_corr_create_validates_before_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p()
    good = dict(k=17, min_high_region=17, max_change=2, further_trim=17, max_tree_nodes=5000000, min_trimmed_len=75)
    for bad in (dict(k=0), dict(k=20), dict(max_tree_nodes=1 << 26), dict(max_tree_nodes=0), dict(min_high_region=0),
                dict(max_change=-1), dict(further_trim=-1), dict(min_trimmed_len=-1)):
        p = capi.CorrParams(**dict(good, **bad))
        assert L.dbgk_corr_create(ctypes.byref(p), 0, ctypes.byref(h)) == capi.ERR_ARG, bad
    assert L.dbgk_corr_create(None, 0, ctypes.byref(h)) == capi.ERR_ARG


def test_binding_covers_the_correct_section():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in ("dbgk_corr_create", "dbgk_corr_destroy", "dbgk_corr_load_bits", "dbgk_corr_seal", "dbgk_corr_from_kfreq",
              "dbgk_corr_table_stats", "dbgk_corr_export_bits", "dbgk_corr_reads", "dbgk_corr_batch_stats"):
        assert n in names and hasattr(capi.lib(), n)
    assert ctypes.sizeof(capi.CorrParams) == 24 and capi.CORR_REC_DTYPE.itemsize == 24
    assert ctypes.sizeof(capi.CorrStats) == 5 * 8 + 3 * 8
    assert capi.lib().dbgk_abi_version() == 7


@pytest.mark.parametrize("d,case", golden_cases(), ids=lambda v: v if isinstance(v, str) else v["name"])
def test_restatement_reproduces_golden(d, case):
    from oracle import oracle_py as orc
    D = os.path.join(GOLDEN, d)
    P = params_of(case)
    bits, hif = orc.kfreq_load_1bit(os.path.join(D, "table.cz"), P.k)
    assert hif == case["hifreq"]
    fa, stat, hits = CR.correct_file(CR.read_records(os.path.join(D, case["reads"]), case["format"]), CR.Table(bits, P.k), P)
    assert stat == open(os.path.join(D, case["name"] + ".correct.stat")).read()
    assert fa == expected_fa(d, case)
    assert hits == case["node_limit_hits"]
