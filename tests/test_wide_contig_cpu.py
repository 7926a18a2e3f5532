"""CPU: the contig stage on 128-bit keys (k = 33..63; parity unpinned above k = 32).  The helper of its GPU tests,
tests/wide_contig_restatement.py, adds nothing to tests/contig_restatement.py while the high word of every key is 0; the two new
symbols of the library; the help text; and the reads of the command-line test, which must give the stage something of every kind
to do at each k."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
import wide_contig_restatement as W  # noqa: E402
from test_contig_cpu import BIN, golden_cases, load_case  # noqa: E402

NEW_SYMBOLS = ("dbgk_wide_contig_create", "dbgk_wide_contig_set_table")
# what the restatement alone removes and reads out from the reads of W.cli_reads() at every k of the command-line test (computed
# with tests/wide_contig_restatement.py on a table built here; the smallest figure over k = 33, 47, 63): a degenerate input would
# make the comparison of tests/test_wide_contig_gpu.py empty
CLI_MINIMA = {"tip": 2, "lowCovEdge": 2, "bubble": 3, "contigs": 4, "branch_ends": 4}


@pytest.mark.parametrize("name", golden_cases())
def test_helper_adds_nothing_while_the_high_word_is_zero(name):
    c = load_case(name)
    o = R.Options.from_args(c["args"])
    want_files, want_err, want_contigs = R.run_stage(R.Table.from_case(c), o)
    t = W.WideTable.from_case(c)
    assert isinstance(t, W.WideTable)
    files, err, contigs = W.run_stage(t, o)
    assert files == want_files and err == want_err and contigs == want_contigs
    assert R.exist_with.__module__ == "contig_restatement"   # the probe of R.linear_seq is the original again


def test_hash_of_a_key_with_a_high_word():
    lo, hi = 0x0123456789abcdef, 0x3
    assert W.hash128(lo) == R.hash_code(lo)
    assert W.hash128((hi << 64) | lo) == R.hash_code(lo ^ R.hash_code(hi)) != R.hash_code(lo)
    t = W.WideTable(11, 40)
    key = (hi << 64) | lo
    assert t.insert(key, 1, 2) == W.hash128(key) % 11 == t.exist(key) and t.exist(lo) == t.size


def test_wide_contig_symbols():
    """fails on a build without the contig stage on 128-bit keys"""
    from dbg_assembly_amd import capi
    L = capi.lib()
    assert L.dbgk_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "dbgk.h")).read()
    bound = [n for n, _, _ in capi.SYMBOLS]
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and ("int %s(" % n) in header and n in bound


def test_wide_create_checks_k_before_any_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p()
    for k in (0, 64):
        assert L.dbgk_wide_contig_create(ctypes.byref(capi.ContigParams(k, 2, 125, 0)), 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_contig_create(ctypes.byref(capi.ContigParams(32, 2, 125, 0)), 0, ctypes.byref(h)) == capi.ERR_ARG   # the narrow range stays
    if L.dbgk_device_count() > 0:
        return
    assert L.dbgk_wide_contig_create(ctypes.byref(capi.ContigParams(63, 2, 125, 0)), 0, ctypes.byref(h)) == capi.ERR_HIP   # no host fall-back
    with pytest.raises(capi.DbgkError) as e:
        capi.ContigBuilder(63, wide=True)
    assert e.value.status == capi.ERR_HIP


def test_help_names_the_wide_range():
    r = subprocess.run([os.path.join(BIN, "debruijn_contig"), "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "33..63" in r.stdout and "k <= 31" in r.stdout


@pytest.mark.parametrize("k", [33, 47, 63])
def test_cli_reads_give_every_pass_something_to_do(k):
    from dbg_assembly_amd import capi
    genome, reads = W.cli_reads()
    assert 4900 <= len(genome) <= 5100 and all(len(r) == W.READ_LEN for r in reads) and len(reads) == len(genome) * W.COVERAGE // W.READ_LEN
    t = W.cli_table(reads, k, capi.find_next_prime_ref(30000))
    files, err, contigs = W.run_stage(t, R.Options.from_args(["-k", str(k)] + W.CLI_ARGS))
    got = W.stage_counts(err, files)
    print(k, got)
    assert any(x >> 64 for x in t.kmer)   # keys with a high word: the ground the reference does not cover
    for name, least in CLI_MINIMA.items():
        assert got[name] >= least, (k, name, got)
