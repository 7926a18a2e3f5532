"""CPU: the ROWS stage (include/dbgk.h) without a device.  Its restatement (tests/maprow_restatement.py), applied to the restated hits
of every golden case of the mapper, gives the files the real reference wrote -- which anchors the row format, the classes, the
counters and the identity's text; the identity rule of csrc/dbgk_maprow_rule.h, compiled alone into a program of its own under
ASan / UBSan, equals `ostream << float` on every pair it is given; the crafted cases (tests/maprow_cases.py) reach what they claim;
the argument checks of the new entry points; the binding."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_restatement as MR  # noqa: E402
import maprow_cases as MC  # noqa: E402
import maprow_restatement as RR  # noqa: E402
from test_map_cpu import CASES, golden_cases  # noqa: E402
from test_map_edges_cpu import EDGE_CASES, edge_expected, edge_golden_cases  # noqa: E402

CSRC = os.path.join(ROOT, "dbg_assembly_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "dbgk.h")).read()


def restated_files(golden_dir, case):
    out = {}
    for name, rows in MC.golden_rows_cases(golden_dir, case):
        e = RR.expected(rows)
        assert e["unprintable"] == 0
        for suffix, data in RR.files_of(rows["mode"], e["streams"], e["counters"]).items():
            out[name + suffix] = data.decode("latin-1")
    return out


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_gives_the_reference_files(case):
    want = MR.expected_outputs(CASES, case)
    got = restated_files(CASES, case)
    assert sorted(got) == sorted(f for f in want if not f.endswith(".lib"))
    for f in got:
        assert got[f] == want[f], f


@pytest.mark.parametrize("case", edge_golden_cases(), ids=lambda c: c["name"])
def test_restatement_gives_the_reference_files_of_the_edge_cases(case):
    want = edge_expected(case)
    got = restated_files(EDGE_CASES, case)
    assert sorted(got) == sorted(f for f in want if not f.endswith(".lib"))
    for f in got:
        assert got[f] == want[f], f


def test_identity_rule_equals_the_stream_in_a_program_of_its_own(tmp_path):
    """all 0 <= m <= a <= 4096, crafted large pairs up to a = 2^31 - 1, a pseudo-random sweep; what the stream prints with an exponent
    (or as no number) must come back unprintable.  The program prints nothing and exits 0."""
    exe = str(tmp_path / "maprow_rule_check")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                         os.path.join(ROOT, "tests", "maprow_rule_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert (r.returncode, r.stdout, r.stderr) == (0, "", ""), (r.stdout[-2000:], r.stderr[-3000:])
    rule = open(os.path.join(CSRC, "dbgk_maprow_rule.h")).read()
    assert "#include <hip" not in rule and "__global__" not in rule and "__device__" not in rule   # the header stands without HIP
    src = open(os.path.join(ROOT, "tests", "maprow_rule_check.cpp")).read()
    assert "check(1, 1 << 24)" in src and "a - 1" in src and "a <= 4096" in src


def test_restated_identity_is_the_mapper_restatement_s():
    for m, a in MC.IDENTITIES:
        p = RR.percent(m, a)
        if a and p is not None:
            assert p.decode() == MR.percent(m, a), (m, a)
    assert RR.percent(1, 1 << 24) == b"100" and RR.percent(1, 10 ** 7) == b"100" and RR.percent(0, 250) == b"100" and RR.percent(250, 250) == b"0"
    assert RR.percent(*MC.UNPRINTABLE) is None and RR.percent(0, 0) is None
    assert "%g" % float(np.float32(0.99999905)) == "0.999999"   # the exponent is the truncated value's: not "1"


def fields_of(case):
    """every row of a case's expected streams (the FASTA stream aside) as its ten fields"""
    e = RR.expected(case)
    rows = []
    for s, text in enumerate(e["streams"]):
        if case["mode"] == RR.READS and s == 2:
            continue
        for line in text.split(b"\n")[:-1]:
            f = line.split(b"\t")
            assert len(f) in (10, 20), line
            rows += [f[:10]] + ([f[10:]] if len(f) == 20 else [])
    return rows


def test_the_crafted_cases_reach_what_they_claim():
    c = MC.cases()
    # the classes: every counter of both modes is hit, a short read / mate is neither written nor counted
    e = RR.expected(c["reads_classes"])
    assert all(e["counters"]) and e["counters"][0] == len(c["reads_classes"]["sides"][0]["recs"]) - 1 and all(e["streams"])
    assert b"r6" not in b"".join(e["streams"]) and e["streams"][1].startswith(b"r3-x\t") and b"\n\t22\t" in e["streams"][1]
    assert b"\n\t23\t" in e["streams"][0] and b">\n" in e["streams"][2] and b"r9-desc\r\t" in e["streams"][0] and b"r10-x\t" in e["streams"][1]
    e = RR.expected(c["pair_classes"])
    assert all(e["counters"]) and e["counters"][0] == len(c["pair_classes"]["sides"][0]["recs"]) - 3 and all(e["streams"])
    gap = e["streams"][2].split(b"\n")
    assert [g.split(b"\t")[0] for g in gap[:5]] == [b"p5/1", b"p6/1", b"p7/2", b"p8/2", b"p15/1"]
    assert b"p11" not in b"".join(e["streams"]) and b"p13" not in b"".join(e["streams"]) and b"p14" not in b"".join(e["streams"])
    assert e["streams"][0].count(b"\n") == e["counters"][1] and e["streams"][1].count(b"\n") == e["counters"][2]
    assert RR.expected(c["pair_classes_fasta"])["streams"] == e["streams"]
    # empty streams beside full ones, n = 0
    assert [bool(s) for s in RR.expected(c["reads_only_1ctg"])["streams"]] == [False, True, False]
    assert [bool(s) for s in RR.expected(c["pair_only_gap"])["streams"]] == [False, False, True]
    assert not any(RR.expected(c["reads_nothing_printed"])["streams"]) and RR.expected(c["reads_nothing_printed"])["counters"][0] == 2
    for name in ("reads_n_0", "pair_n_0"):
        assert RR.expected(c[name]) == {"streams": [b"", b"", b""], "counters": [0] * 5, "unprintable": 0}
    # a header that ends the text
    for name in ("reads_header_ends_the_text_2ctg", "reads_header_ends_the_text_1ctg", "pair_header_ends_the_text"):
        for s in c[name]["sides"]:
            r = s["recs"][-1]
            assert int(r["head_pos"]) + int(r["head_len"]) == len(s["text"]) and not s["text"].endswith(b"\n")
    assert RR.expected(c["reads_header_ends_the_text_2ctg"])["streams"][2].endswith(b">last-one\n\n")
    assert RR.expected(c["reads_header_ends_the_text_1ctg"])["streams"][1].startswith(b"z\t0\t")
    # every digit count of every number: PAIR reaches ten everywhere, READS seven in the read's length (its bases are real)
    digits = [set() for _ in range(10)]
    for f in fields_of(c["digits_pair"]):
        for k in (1, 2, 3, 5, 6, 7):
            digits[k].add(len(f[k]))
    assert all(digits[k] == set(range(1, 11)) for k in (1, 2, 3, 5, 6, 7)), digits
    digits = [set() for _ in range(10)]
    for f in fields_of(c["digits_reads"]):
        for k in (1, 2, 3, 5, 6, 7):
            digits[k].add(len(f[k]))
    assert digits[1] == set(range(1, 8)) and all(max(digits[k]) == 10 for k in (2, 3, 5, 6, 7)), digits
    assert max(len(q) for q in RR.expected(c["digits_reads"])["streams"][2].split(b"\n")) == 10 ** 6 + 7
    # the identity: 0, 100, one to six significant digits, eleven bytes, the carry into the next power of ten
    texts = {f[9][:-1] for f in fields_of(c["identities"])}
    assert {b"0", b"100", b"50", b"75", b"87.5", b"93.75", b"96.875", b"98.4375", b"66.6667", b"33.3333"} <= texts
    assert {len(t.replace(b".", b"").lstrip(b"0").rstrip(b"0") or b"0") for t in texts} >= {1, 2, 3, 4, 5, 6}
    assert max(len(t) for t in texts) == RR.IDENT_MAX and any(t.startswith(b"0.000") for t in texts) and any(t.startswith(b"0.0") for t in texts)
    assert float(np.float32(1.0 - float(np.float32(1) / np.float32(10 ** 7))) * np.float32(100)) < 99.99999   # 99.99998: six digits carry to 100
    assert len(texts) > 60 and all(a >= 2 ** 23 for m, a in MC.IDENTITIES if RR.percent(m, a) is None)   # (those are left out of the case)
    for name in ("reads_unprintable", "pair_unprintable"):
        e = RR.expected(c[name])
        assert e["unprintable"] == 1 and e["streams"] == [b"", b"", b""] and e["counters"][0] > 10
    # where rows and streams end
    ends, at = [], 0
    for line in RR.expected(c["vector_ends"])["streams"][1].split(b"\n")[:-1]:
        at += len(line) + 1
        ends.append(at % 16)
    assert ends == [0, 1, 15, 0, 1, 0, 0, 15, 8]
    tile = int(re.search(r"#define\s+DBGK_MAPROW_TILE\s+(\d+)", HEADER).group(1))
    assert tile == MC.TILE
    for name, stream, total in (("reads_1ctg_of_%d_bytes", 1, None), ("reads_2ctg_of_%d_bytes", 0, None), ("pair_gap_of_%d_bytes", 2, None)):
        for total in (tile, tile + 1):
            assert len(RR.expected(c[name % total])["streams"][stream]) == total
    assert len(RR.expected(c["pair_2ctg_of_4096_bytes"])["streams"][0]) == tile and len(RR.expected(c["pair_1ctg_of_8192_bytes"])["streams"][1]) == 2 * tile
    # more than one workgroup round of the segment kernel (256 slots), more than one tile in every stream
    for name in ("reads_random", "pair_random"):
        e = RR.expected(c[name])
        assert 2 * len(c[name]["sides"][0]["recs"]) > 4 * 256 and all(len(s) > 2 * tile for s in e["streams"][:1]) and all(e["counters"])
    kernels = open(os.path.join(CSRC, "dbgk_maprow.h")).read()
    assert "kSlot = 112, kSegB = 48, kLenAt = 44" in kernels
    assert RR.HIT_DTYPE.itemsize == 32 and RR.REC_DTYPE.itemsize == 24


def test_arguments_are_refused_before_any_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    h, p, u = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
    info = capi.MapRowInfo()
    side = (capi.MapRowSide * 2)()
    for mode, delims, r, dev in ((0, b"@ \t", 250, 0), (3, b"@ \t", 250, 0), (capi.MAPROW_READS, None, 250, 0), (capi.MAPROW_READS, b"", 250, 0),
                                 (capi.MAPROW_READS, b"x" * 17, 250, 0), (capi.MAPROW_PAIR, b"@\xff", 250, 0), (capi.MAPROW_PAIR, b"@ \t", -1, 0),
                                 (capi.MAPROW_PAIR, b"@ \t", 250, -1)):
        assert L.dbgk_maprow_create(mode, delims, r, dev, ctypes.byref(h)) == capi.ERR_ARG, (mode, delims, r, dev)
        assert not h.value
    assert L.dbgk_maprow_create(capi.MAPROW_READS, b"@ \t", 250, 0, None) == capi.ERR_ARG
    assert L.dbgk_maprow_destroy(None) == capi.ERR_ARG
    off = (ctypes.c_uint64 * 2)(0, 4)
    lens = (ctypes.c_uint32 * 1)(100)
    assert L.dbgk_maprow_set_contigs(None, b"ctg1", off, lens, 1) == capi.ERR_ARG
    assert L.dbgk_maprow_take_hits(None, 0, None) == capi.ERR_ARG
    assert L.dbgk_maprow_rows_device(None, side, 0, ctypes.byref(info)) == capi.ERR_ARG
    assert L.dbgk_maprow_rows(None, side, 0, ctypes.byref(info)) == capi.ERR_ARG
    assert L.dbgk_maprow_device(None, 0, ctypes.byref(p), ctypes.byref(u)) == capi.ERR_ARG
    assert L.dbgk_maprow_results(None, 0, None, 0) == capi.ERR_ARG
    assert L.dbgk_map_hits_device(None, ctypes.byref(p), ctypes.byref(u)) == capi.ERR_ARG
    assert L.dbgk_map_reads_device_keep(None, None, None, 0, 0, 0) == capi.ERR_ARG


def test_binding_covers_the_rows_section():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    declared = set(re.findall(r"\b(dbgk_maprow_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)))
    assert declared == {"dbgk_maprow_" + f for f in ("create", "destroy", "set_contigs", "take_hits", "rows_device", "rows", "device", "results")}
    for n in declared | {"dbgk_map_hits_device", "dbgk_map_reads_device_keep"}:
        assert n in names and hasattr(capi.lib(), n)
    assert ctypes.sizeof(capi.MapRowInfo) == 8 * (1 + 5 + 3 + 1) + 2 * 8 and ctypes.sizeof(capi.MapRowSide) == 6 * 8
    assert (capi.MAPROW_READS, capi.MAPROW_PAIR, capi.MAPROW_STREAMS, capi.MAPROW_TILE) == (RR.READS, RR.PAIR, 3, MC.TILE)
    for k, v in (("DBGK_MAPROW_READS", 1), ("DBGK_MAPROW_PAIR", 2), ("DBGK_MAPROW_STREAMS", 3)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % k, HEADER).group(1)) == v
    assert capi.MAP_HIT_DTYPE == RR.HIT_DTYPE and capi.PARSE_REC_DTYPE == RR.REC_DTYPE
    for m in ("set_contigs", "take_hits", "rows", "rows_device", "results", "device"):
        assert callable(getattr(capi.RowWriter, m))
    assert "keep" in capi.Mapper.map_device.__code__.co_varnames and callable(capi.Mapper.hits_device)
