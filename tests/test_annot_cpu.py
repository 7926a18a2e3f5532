"""CPU: the annotation of the corrector's headers.  Its restatement (tests/annot_restatement.py) applied to the records
tests/correct_restatement.py computes, joined with the input headers and the restated sequences, gives the text of every golden
.correct.fa.gz the real reference wrote -- which anchors the literals; the crafted cases (tests/annot_cases.py) are
self-consistent and reach the bound include/dbgk.h declares; the two multiply-shift constants of the write kernel divide as they
claim; the argument checks of the new entry points; the binding."""
import ctypes
import gzip
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import annot_cases as AC  # noqa: E402
import annot_restatement as AR  # noqa: E402
import corr_compact_restatement as CC  # noqa: E402
import correct_edge_cases as E  # noqa: E402
import correct_restatement as CR  # noqa: E402
from test_correct_cpu import GOLDEN, expected_fa, golden_cases, params_of  # noqa: E402

EDGES = os.path.join(GOLDEN, "correct_edges")
PINNED = [s.name for s in E.scenarios() if s.pinned]
HEADER = open(os.path.join(ROOT, "include", "dbgk.h")).read()
KERNELS = open(os.path.join(ROOT, "dbg_assembly_amd", "csrc", "dbgk_annot.h")).read()


def text_of(heads, outs, rows):
    """header + restated suffix + "\\n" + the compact record + "\\n" for every read"""
    offsets = np.zeros(len(outs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in outs])
    rec = CC.records_of(rows)
    bases, coff, _ = CC.compact(np.frombuffer(b"".join(outs), dtype=np.uint8), offsets, rec)
    plane, soff = AR.suffixes(rec, np.diff(coff.astype(np.int64)))
    return b"".join(h + s + b"\n" + b + b"\n" for h, s, b in zip(heads, AR.split(plane, soff), CC.as_lines(bases, coff)))


def golden_k12():
    return [(d, c) for d, c in golden_cases() if d == "correct_k12"]


@pytest.mark.parametrize("d,case", golden_k12(), ids=lambda v: v if isinstance(v, str) else v["name"])
def test_restated_suffixes_give_the_golden_text_k12(d, case):
    from oracle import oracle_py as orc
    D = os.path.join(GOLDEN, d)
    P = params_of(case)
    bits, _ = orc.kfreq_load_1bit(os.path.join(D, "table.cz"), P.k)
    T = CR.Table(bits, P.k)
    heads, outs, rows = [], [], []
    for head, seq in CR.read_records(os.path.join(D, case["reads"]), case["format"]):
        read, one, multi, deleted, lt, rt, hits = CR.correct_one_read(seq, T, P)
        heads.append(b">" + head[1:])
        outs.append(read)
        rows.append((one, multi, deleted, lt, rt, hits))
    assert len(heads) > 100
    assert text_of(heads, outs, rows) == expected_fa(d, case)


@pytest.mark.parametrize("name", PINNED)
def test_restated_suffixes_give_the_golden_text_edges(name):
    s, rs = E.scenario(name), E.restated(name)
    heads = [b">" + h[1:] for h in E.headers(s)]
    got = text_of(heads, [r["out"] for r in rs], [(r["one_base"], r["tree"], r["deleted"], r["lt"], r["rt"], r["hits"]) for r in rs])
    assert got == gzip.open(os.path.join(EDGES, name + ".correct.fa.gz"), "rb").read()


def test_the_crafted_cases_are_self_consistent_and_reach_the_declared_bound():
    bound = int(re.search(r"#define\s+DBGK_CORR_ANNOT_MAX\s+(\d+)", HEADER).group(1))
    assert bound == AR.MAX_SUFFIX == 77 + 43
    cases = dict(AC.cases(), cpu_only=AC.CPU_ONLY)
    longest, shortest = 0, bound
    for name, c in cases.items():
        plane, off = AC.expected(c)
        n = len(c["rec"])
        assert len(off) == n + 1 and off[0] == 0 and int(off[-1]) == plane.size, name
        parts = AR.split(plane, off)
        for r, L, s in zip(c["rec"], c["F"] if "F" in c else AC.compact_lengths(c), parts):
            m = re.fullmatch(rb"\tModifiedBaseNum: (\d+)\tFinalReadLength: (\d+)\tLeftEndTrim: (\d+)\tRightEndTrim: (\d+)\tIsDeleted: (\d+)", s)
            assert m, (name, s)
            assert [int(v) for v in m.groups()] == [(int(r["one_base"]) + int(r["tree"])) % 2 ** 32, int(L), int(r["left_trim"]), int(r["right_trim"]),
                                                    int(r["deleted"])]
            assert not any(v.startswith(b"0") and v != b"0" for v in m.groups())
        if parts:
            longest, shortest = max(longest, max(map(len, parts))), min(shortest, min(map(len, parts)))
    assert longest == bound and shortest == AC.MIN_SUFFIX == 82
    assert max(len(s) for s in AR.split(*AC.expected(AC.CPU_ONLY))) == bound
    # on the device a suffix stays below it: ten digits in both trims leave the length one
    assert max(len(s) for name, c in AC.cases().items() for s in AR.split(*AC.expected(c))) == bound - 9
    assert {len(s) for s in AR.split(*AC.expected(AC.cases()["all_minimal"]))} == {AC.MIN_SUFFIX}
    for extra in (0, 1):
        assert int(AC.expected(AC.cases()["suffix_bytes_16384%+d" % extra])[1][-1]) == 16384 + extra
    c = AC.cases()
    assert [len(c["n_%d" % n]["rec"]) for n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513)] == [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513]
    assert AC.GROUP == int(re.search(r"kEmitBlock = (\d+);", open(os.path.join(ROOT, "dbg_assembly_amd", "csrc", "dbgk_emit.h")).read()).group(1))
    assert "constexpr int kAnnotGroup = kEmitBlock;" in KERNELS
    assert list(c)[-2:] == ["large", "small_after_large"] and len(c["large"]["rec"]) > 50 * AC.GROUP
    wraps = AR.split(*AC.expected(c["sum_that_wraps"]))
    assert [s.split(b"\t")[1] for s in wraps] == [b"ModifiedBaseNum: 0", b"ModifiedBaseNum: 0", b"ModifiedBaseNum: 4", b"ModifiedBaseNum: 4294967294"]
    digits = {f: set() for f in range(5)}
    for name, case in c.items():
        for s in AR.split(*AC.expected(case)):
            for f, v in enumerate(re.findall(rb": (\d+)", s)):
                digits[f].add(len(v))
    assert digits[0] == digits[2] == digits[3] == set(range(1, 11)) and digits[1] == set(range(1, 9)) and digits[4] == {1, 2, 3}


def test_the_literals_of_the_kernel_are_the_restatement_s():
    lits = re.findall(r'DBGK_ANNOT_LITERAL\(\w+, "((?:[^"\\]|\\.)*)"\);', KERNELS)
    assert tuple(x.encode("ascii").decode("unicode_escape").encode("ascii") for x in lits) == AR.LITERALS
    assert sum(len(x) for x in AR.LITERALS) == 77 and len(AR.LITERALS[0]) >= 15
    src = open(os.path.join(ROOT, "dbg_assembly_amd", "host", "correct_error_reads.cpp")).read()
    assert '"\\tModifiedBaseNum: %u\\tFinalReadLength: %llu\\tLeftEndTrim: %u\\tRightEndTrim: %u\\tIsDeleted: %u\\n"' in src


def test_the_multiply_shift_constants_divide_exactly():
    """x / 10 = x * 0xCCCCCCCD >> 35 and x / 10^8 = x * 0xABCC7712 >> 58 for every 32-bit x: floor(x * m / 2^s) = floor(x / d) holds
    when m * d - 2^s = e >= 0 and x * e < 2^s for the largest x (then the error term stays below one step of 1 / d)"""
    for m, s, d in ((0xCCCCCCCD, 35, 10), (0xABCC7712, 58, 10 ** 8)):
        assert "0x%Xull) >> %d" % (m, s) in KERNELS
        e = m * d - 2 ** s
        assert 0 <= e and (2 ** 32 - 1) * e < 2 ** s
        xs = [0, 1, d - 1, d, d + 1, 2 ** 32 - 1] + [k * d + j for k in range(1, 2 ** 32 // d + 1, max(1, 2 ** 32 // d // 50)) for j in (-1, 0, 1) if k * d + j < 2 ** 32]
        assert all(x * m >> s == x // d for x in xs)


def test_null_arguments_are_refused_before_any_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    info, fi = capi.CorrAnnotInfo(), capi.FmtInfo()
    p, u = ctypes.c_void_p(), ctypes.c_uint64()
    assert L.dbgk_corr_annot(None, ctypes.byref(info)) == capi.ERR_ARG
    assert L.dbgk_corr_annot_device(None, ctypes.byref(p), ctypes.byref(p), ctypes.byref(u), ctypes.byref(u)) == capi.ERR_ARG
    assert L.dbgk_corr_annot_results(None, None, None) == capi.ERR_ARG
    assert L.dbgk_fmt_records_device_suffix(None, None, 0, None, None, None, None, 0, None, None, ctypes.byref(fi)) == capi.ERR_ARG


def test_binding_covers_the_annotation():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in ("dbgk_corr_annot", "dbgk_corr_annot_device", "dbgk_corr_annot_results", "dbgk_fmt_records_device_suffix"):
        assert n in names and hasattr(capi.lib(), n)
    assert ctypes.sizeof(capi.CorrAnnotInfo) == 4 * 8 and capi.CORR_ANNOT_MAX == AR.MAX_SUFFIX
    for m in ("annotate", "annotate_device"):
        assert callable(getattr(capi.Corrector, m))
    assert capi.DeviceSuffixes._fields == ("d_suffix", "d_offsets", "n", "n_bytes")
