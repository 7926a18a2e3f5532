"""CPU: the restatement of the contig stage (tests/contig_restatement.py) against what the real reference program wrote for the
cases of tests/golden/contig_cases (made by tests/golden/make_contig_golden.py), the CONTIG symbols of the library, and the help
text of bin/debruijn_contig."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402

CASES = os.path.join(ROOT, "tests", "golden", "contig_cases")
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
SUFFIXES = R.SUFFIXES


def golden_cases():
    return sorted(f[:-4] for f in os.listdir(CASES) if f.endswith(".npz"))


def load_case(name):
    return R.load_case(os.path.join(CASES, name + ".npz"))


def in_order(lines, text):
    """every line of `lines` appears in text, in this order"""
    pos = 0
    for ln in lines:
        at = text.find(ln + "\n", pos)
        if at < 0:
            return ln
        pos = at + len(ln) + 1
    return None


def stage_lines(stderr):
    """the stage's lines, without empty ones"""
    return [ln for ln in stderr.split("\n") if ln.strip()]


@pytest.mark.parametrize("name", golden_cases())
def test_restatement_reproduces_the_reference(name):
    c = load_case(name)
    t = R.Table.from_case(c)
    files, err, contigs = R.run_stage(t, R.Options.from_args(c["args"]))
    assert sorted(files) == sorted(c["files"])
    for s in files:
        assert files[s] == c["files"][s], (name, s)
    assert in_order(stage_lines(err), c["stderr"] + "\n") is None
    # the cap on the hand-off: what make_contig_golden.py recorded is what the table shows
    host = R.order_dependent_nodes(t)
    assert sum(1 for x in contigs if x["anchor"] in host) == c["shows"]["host_walked_contigs"]
    if name[0] not in "gh":
        assert c["shows"]["host_walked_contigs"] == 0


def test_std_sort_restatement_is_a_sort_and_keeps_short_inputs_stable():
    import random
    rng = random.Random(3)
    for n in (0, 1, 5, 16, 17, 40, 300):
        a = [(rng.randrange(6), i) for i in range(n)]
        b = R.std_sort(list(a), lambda x, y: y[0] < x[0])
        assert sorted(b) == sorted(a) and all(b[i][0] >= b[i + 1][0] for i in range(n - 1))
        if n <= 16:   # insertion sort only
            assert b == sorted(a, key=lambda x: -x[0])


def test_contig_symbols_and_abi():
    from dbg_assembly_amd import capi
    L = capi.lib()
    assert L.dbgk_abi_version() == 7
    names = [n for n, _, _ in capi.SYMBOLS if n.startswith("dbgk_contig_")]
    assert sorted(names) == ["dbgk_contig_create", "dbgk_contig_destroy", "dbgk_contig_read_out", "dbgk_contig_results", "dbgk_contig_set_table",
                             "dbgk_contig_summary_get", "dbgk_contig_timing_get"]
    header = open(os.path.join(ROOT, "include", "dbgk.h")).read()
    for n in names:
        assert hasattr(L, n) and ("int %s(" % n) in header
    assert capi.CONTIG_RECORD_DTYPE.itemsize == 48
    # the stage is not part of the host library: a program that links the reference's contig.cpp next to it keeps its own
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dbg_assembly_amd", "lib", "libdbgasm_host.so")], capture_output=True, text=True).stdout
    assert "run_contig_stage" not in out and "KmerFreqCutoff" not in out


def test_help_lists_every_option():
    r = subprocess.run([os.path.join(BIN, "debruijn_contig"), "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in "krfotilebDTIPWCGBULEM":
        assert ("   -%s <" % opt) in r.stdout, opt
    assert "debruijn_contig   <reads_file.lib>" in r.stdout and "-h          this help" in r.stdout and "Version: 1.0 (gfx950)" in r.stdout
    assert "DBGK_LAYOUT=ref" in r.stdout and "[125]" in r.stdout
