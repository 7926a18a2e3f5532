"""CPU: tests/format_restatement.py, the plain statement of the FORMAT stage's rule, anchored to code and files that are already
pinned -- the cleaners' writer RecordBatch::write through tests/format_write_test.cpp on the crafted FASTQ batches of
tests/format_cases.py, and bytes the real reference wrote: every CLEAN golden output (FASTQ) and every .correct.fa golden (FASTA)
parsed by the PARSE restatement and formatted again is the file itself.  Then the FORMAT section's symbols, constants, struct size
and the argument checks that need no device."""
import ctypes as C
import glob
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_restatement as CR  # noqa: E402
import format_cases as FC  # noqa: E402
import format_restatement as FR  # noqa: E402
import parse_restatement as PR  # noqa: E402
from dbg_assembly_amd import capi  # noqa: E402

HOST = os.path.join(ROOT, "dbg_assembly_amd", "host")
LIB = os.path.join(ROOT, "dbg_assembly_amd", "lib")
NAMES = ("dbgk_fmt_create", "dbgk_fmt_destroy", "dbgk_fmt_records_device", "dbgk_fmt_records", "dbgk_fmt_results", "dbgk_fmt_device",
         "dbgk_parse_recs_device", "dbgk_parse_text_device")


@pytest.fixture(scope="module")
def cases():
    return FC.cases()


@pytest.fixture(scope="module")
def write_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("format_write") / "format_write_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "format_write_test.cpp"),
                    "-o", out, "-L" + LIB, "-ldbgk", "-lz", "-Wl,-rpath," + LIB], check=True)
    return out


def test_the_restatement_equals_the_cleaners_writer_on_the_crafted_batches(write_exe, cases, tmp_path):
    env = {k: v for k, v in os.environ.items() if k != "DBGK_GZ"}
    seen = 0
    for name, case in cases.items():
        if case["fmt"] != FC.FASTQ or case["marker"]:
            continue   # the writer knows FASTQ and no marker
        heads, reads, quals = FR.pieces_of(case["text"], case["recs"], case["bases"], case["quals"], case["offsets"])
        if case["suffixes"] is not None:   # the programs append the annotation to the header before they write
            heads = [h + s for h, s in zip(heads, case["suffixes"])]
        src, dst = str(tmp_path / "records"), str(tmp_path / "out.gz")
        with open(src, "wb") as f:
            for entry in (e for rec in zip(heads, reads, quals) for e in rec):
                f.write(b"%d\t%s\n" % (len(entry), entry))
        r = subprocess.run([write_exe, src, dst], capture_output=True, check=True, env=env)
        assert int(r.stdout) == len(heads), name
        assert gzip.decompress(open(dst, "rb").read()) == FC.expected(case)[0], name
        seen += 1
    assert seen >= 20


def test_the_sweep_covers_every_residue_and_the_cases_their_names(cases):
    for tag in ("fastq", "fasta"):
        assert FC.covers_every_residue(cases["sweep_0_100_" + tag])
        c = cases["sweep_0_100_" + tag]
        lens = np.diff(c["offsets"].astype(np.int64))
        assert set(lens.tolist()) == set(c["recs"]["head_len"].tolist()) == {len(s) for s in c["suffixes"]} == set(range(101))
        assert int(c["offsets"][0]) % 16 and c["recs"]["head_pos"][0] == 0
        text, info = FC.expected(cases["run_of_3T_emptied_records_" + tag])
        assert info["n_records"] == 3 * FC.T + 2 and info["seq_bytes"] == 301
        _, info = FC.expected(cases["pieces_of_3T_and_100_" + tag])
        assert info["out_bytes"] > 9 * FC.T
        assert {len(cases["header_ends_the_text_%d_%s" % (m, tag)]["text"]) % 4 for m in (2, 3, 0)} == {2, 3, 0}
    assert (cases["sweep_0_100_fastq"]["recs"]["seq_pos"] == FC.JUNK).all()
    a, b = FC.expected(cases["marker_3e_fastq"])[0], FC.expected(cases["marker_40_fastq"])[0]
    assert len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 60 - 12   # (12 headers are empty: nothing to replace)


def clean_goldens():
    return [c["name"] for c in CR.golden_cases(FC.CLEAN)]


def correct_goldens():
    return sorted(os.path.relpath(p, os.path.join(ROOT, "tests", "golden")) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*", "*.correct.fa.gz")))


def round_trip(x, fmt):
    got = PR.parse(x, fmt, with_quals=False)
    # the precondition of the round trip: the file ends with a newline and every line of it belongs to a record
    assert (not x or x.endswith(b"\n")) and got["info"]["ignored_lines"] == 0 and got["info"]["n_lines"] == (4 if fmt == 1 else 2) * len(got["records"])
    heads, reads, quals = ([r[i] for r in got["records"]] for i in range(3))
    text, info = FR.format_text(fmt, heads, reads, quals if fmt == 1 else None)
    assert text == x and info["out_bytes"] == len(x) and info["n_records"] == got["info"]["n_records"]
    return len(heads)


@pytest.mark.parametrize("name", clean_goldens())
def test_a_clean_golden_output_parsed_and_formatted_again_is_the_file(name):
    case = [c for c in CR.golden_cases(FC.CLEAN) if c["name"] == name][0]
    n = round_trip(CR.expected_outputs(FC.CLEAN, case)["out"].encode("latin-1"), 1)
    assert (n == 0) == (case["input"] == "norecords.fq")


def test_the_corrector_golden_outputs_parsed_and_formatted_again_are_the_files():
    names = correct_goldens()
    assert len(names) >= 5
    assert sum(round_trip(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", n), "rb").read()), 2) for n in names) > 1000


def test_the_library_exports_the_section_and_the_binding_has_it():
    L = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    for name in NAMES:
        assert hasattr(L, name), "libdbgk.so does not export %s" % name
        assert name in bound, name
    header = open(os.path.join(ROOT, "include", "dbgk.h")).read()
    assert "#define DBGK_FMT_TILE %d" % capi.FMT_TILE in header and capi.FMT_TILE == FC.T
    assert C.sizeof(capi.FmtInfo) == 5 * 8 + 2 * 8
    for f in ("n_records", "out_bytes", "head_bytes", "suffix_bytes", "seq_bytes", "ms_scan", "ms_gather"):
        assert f in header.split("typedef struct dbgk_fmt_info {")[1].split("} dbgk_fmt_info;")[0]
    assert tuple(f for f, _ in capi.FmtInfo._fields_[:5]) == FR.COUNTERS
    for f in ("format", "format_device", "device", "results", "close", "__enter__", "__exit__"):
        assert callable(getattr(capi.Formatter, f))


def test_the_argument_checks_that_need_no_device():
    L = capi.lib()
    h = C.c_void_p()
    for fmt, marker in ((0, 0), (3, 0), (1, -1), (1, 256)):
        assert L.dbgk_fmt_create(fmt, marker, 0, C.byref(h)) == capi.ERR_ARG and not h.value
    assert L.dbgk_fmt_create(1, 0, -1, C.byref(h)) == capi.ERR_ARG
    assert L.dbgk_fmt_create(1, 0, 0, None) == capi.ERR_ARG
    info, p, n = capi.FmtInfo(), C.c_void_p(), C.c_uint64()
    assert L.dbgk_fmt_destroy(None) == capi.ERR_ARG
    assert L.dbgk_fmt_records(None, None, 0, None, None, None, None, 0, None, None, C.byref(info)) == capi.ERR_ARG
    assert L.dbgk_fmt_records_device(None, None, 0, None, None, None, None, 0, None, None, C.byref(info)) == capi.ERR_ARG
    assert L.dbgk_fmt_results(None, None, 0) == capi.ERR_ARG
    assert L.dbgk_fmt_device(None, C.byref(p), C.byref(n)) == capi.ERR_ARG
    assert L.dbgk_parse_recs_device(None, C.byref(p)) == capi.ERR_ARG
    assert L.dbgk_parse_text_device(None, C.byref(p), C.byref(n)) == capi.ERR_ARG
