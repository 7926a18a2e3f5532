"""CPU: the cleaner's output stage.  Its numpy restatement (tests/clean_compact_restatement.py) applied to what
tests/clean_restatement.py computes gives, for every golden the real reference wrote, exactly lines 2 and 4 of every record of
out.gz and the integer columns of out.stat, and for every pinned edge scenario what Cleaner.trim_*'s rule gives; the length rule
the kernel and the host share (csrc/dbgk_clean_rule.h) as a program of its own under the sanitizers; the argument checks of the
new entry points; the binding."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_compact_restatement as CC  # noqa: E402
import clean_edge_cases as E  # noqa: E402
import clean_restatement as CR  # noqa: E402

CASES = os.path.join(ROOT, "tests", "golden", "clean_cases")
PINNED = [s.name for s in E.scenarios() if E.pinned(s)]
NEW = ("dbgk_clean_lowqual_device", "dbgk_clean_adapter_device", "dbgk_clean_compact", "dbgk_clean_compact_from",
       "dbgk_clean_compact_results", "dbgk_clean_compact_device", "dbgk_push_cleaned")


def restated_records(case, batch):
    o = batch["opts"]
    if batch["kind"] == CC.ADAPTER:
        adapters = CR.case_adapters(CASES, case)
        return CC.hits_of([CR.first_hit(s.decode("latin-1"), adapters, o["-s"]) for s in batch["reads"]])
    table = CR.error_table(o["-q"])
    return CC.blocks_of([CR.lowqual_block(s.decode("latin-1"), q.decode("latin-1"), o["-e"], o["-q"], table)
                         for s, q in zip(batch["reads"], batch["quals"])])


@pytest.mark.parametrize("case", CR.golden_cases(CASES), ids=lambda c: c["name"])
def test_compaction_of_the_restatement_gives_lines_2_and_4_and_the_stat_of_the_golden(case):
    b = CC.golden_batch(CASES, case)
    bases, offsets = CC.pack(b["reads"])
    quals, _ = CC.pack(b["quals"])
    rec = restated_records(case, b)
    out_b, out_q, coff, cnt = CC.compact(b["kind"], bases, quals, offsets, rec, b["opts"]["-q"], b["opts"]["-r"])
    assert CC.as_lines(out_b, coff) == b["lines2"]
    assert CC.as_lines(out_q, coff) == b["lines4"]
    assert cnt == b["stat"]
    if "norecords" in case["name"]:
        assert cnt["reads"] == 0 and coff.tolist() == [0] and out_b.size == 0 and out_q.size == 0


def edge_batch(s):
    """a scenario of clean_edge_cases -> (kind, reads, quals, shift)"""
    if isinstance(s, E.AdapterScenario):
        return CC.ADAPTER, list(s.reads), [b"I" * len(r) for r in s.reads], 33
    return CC.LOWQUAL, [b for b, _ in s.reads], [q for _, q in s.reads], s.shift


@pytest.mark.parametrize("name", PINNED)
def test_compaction_of_the_edge_scenarios_gives_what_the_trim_rule_gives(name):
    s = E.scenario(name)
    kind, reads, quals, shift = edge_batch(s)
    rows = E.restated(name)
    rec = CC.hits_of(rows) if kind == CC.ADAPTER else CC.blocks_of(rows)
    bases, offsets = CC.pack(reads)
    qplane, _ = CC.pack(quals)
    for min_len in (0, 10):
        want2, want4, want_c = CC.trim_rule(kind, reads, quals, rows, shift, min_len)
        out_b, out_q, coff, cnt = CC.compact(kind, bases, qplane, offsets, rec, shift, min_len)
        assert CC.as_lines(out_b, coff) == want2 and CC.as_lines(out_q, coff) == want4 and cnt == want_c, (name, min_len)


def test_the_two_programs_count_clean_reads_differently():
    """min_len 0 and an empty read: clean_adapter counts it as clean, clean_lowqual does not; and a record that points outside its
    read keeps nothing"""
    bases, offsets = CC.pack([b"ACGT", b"", b"ACGTACGT"])
    hits = CC.hits_of([(-1, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0), (0, 5, 1, 5, 1, 5)])
    blocks = CC.blocks_of([(0.0, 1, 4, 0), (0.0, 0, 0, 0), (1.0, 0, 0, 1)])
    assert CC.compact(CC.ADAPTER, bases, None, offsets, hits, 33, 0)[3]["clean_reads"] == 3
    assert CC.compact(CC.LOWQUAL, bases, None, offsets, blocks, 33, 0)[3]["clean_reads"] == 1
    outside = CC.hits_of([(0, 5, 6, 6, 1, 1), (0, 5, 2, 2, 1, 1), (0, 5, 0, 0, 1, 1)])
    assert CC.cuts(CC.ADAPTER, offsets, outside)[1].tolist() == [0, 0, 0]
    outside = CC.blocks_of([(0.0, 2, 4, 1), (0.0, 1, 1, 1), (0.0, 9, -1, 1)])
    assert CC.cuts(CC.LOWQUAL, offsets, outside)[1].tolist() == [0, 0, 0]


def test_length_rule_and_offset_checks_under_the_sanitizers(tmp_path):
    """csrc/dbgk_clean_rule.h, the HIP-free header the length kernel and the host's checks share, compiled with the system C++
    compiler and -fsanitize=address,undefined into a program with its own main and run as such, in the environment as it is"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no system C++ compiler"
    exe = tmp_path / "clean_rule_test"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts whatever else the process loads
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dbg_assembly_amd", "csrc"),
                    os.path.join(ROOT, "tests", "clean_rule_test.cpp"), "-o", str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("checks ok") and int(r.stdout.split()[0]) >= 40


def test_a_null_handle_is_an_argument_error_from_every_new_entry_point():
    """fails on a build without the feature: the symbols do not exist"""
    from dbg_assembly_amd import capi
    L = capi.lib()
    info = capi.CleanCompactInfo()
    p, u = ctypes.c_void_p(), ctypes.c_uint64()
    off = (ctypes.c_uint64 * 1)(0)
    out = (ctypes.c_int32 * 8)()
    assert L.dbgk_clean_lowqual_device(None, None, None, off, 0, 0.001, 33, out) == capi.ERR_ARG
    assert L.dbgk_clean_adapter_device(None, None, None, off, 0, out) == capi.ERR_ARG
    assert L.dbgk_clean_compact(None, 75, ctypes.byref(info)) == capi.ERR_ARG
    assert L.dbgk_clean_compact_from(None, capi.CLEAN_KIND_ADAPTER, None, None, off, None, 0, 33, 75, ctypes.byref(info)) == capi.ERR_ARG
    assert L.dbgk_clean_compact_results(None, None, None, None) == capi.ERR_ARG
    assert L.dbgk_clean_compact_device(None, ctypes.byref(p), ctypes.byref(p), ctypes.byref(p), ctypes.byref(u), ctypes.byref(u)) == capi.ERR_ARG
    assert L.dbgk_push_cleaned(None, None) == capi.ERR_ARG


def test_binding_covers_the_output_stage():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in NEW:
        assert n in names and hasattr(capi.lib(), n)
    header = open(os.path.join(ROOT, "include", "dbgk.h")).read()
    body = re.search(r"typedef struct dbgk_clean_compact_info \{(.*?)\} dbgk_clean_compact_info;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, ns in re.findall(r"\b(uint64_t|double)\s+([^;]+);", body) for n in ns.split(",")]
    assert [n for _, n in fields] == [f for f, _ in capi.CleanCompactInfo._fields_]
    assert [n for t, n in fields if t == "uint64_t"] == list(CC.COUNTERS)
    assert ctypes.sizeof(capi.CleanCompactInfo) == 8 * len(fields) == 80
    assert CC.HIT_DTYPE == capi.ADAPTER_HIT_DTYPE and CC.BLOCK_DTYPE == capi.LOWQUAL_BLOCK_DTYPE
    assert "#define DBGK_CLEAN_COMPACT_TILE %d\n" % capi.CLEAN_COMPACT_TILE in header
    for name, value in (("LOWQUAL", capi.CLEAN_KIND_LOWQUAL), ("ADAPTER", capi.CLEAN_KIND_ADAPTER)):
        assert re.search(r"#define DBGK_CLEAN_KIND_%s %d\b" % (name, value), header)
    assert (CC.LOWQUAL, CC.ADAPTER) == (capi.CLEAN_KIND_LOWQUAL, capi.CLEAN_KIND_ADAPTER)
    assert capi.CLEAN_COMPACT_TILE % 16 == 0 and capi.lib().dbgk_abi_version() == 7
    for m in ("lowqual_device", "adapter_device", "compact", "compact_from", "compact_to_host", "compact_device"):
        assert callable(getattr(capi.Cleaner, m))
    assert callable(capi.Graph.push_cleaned)
