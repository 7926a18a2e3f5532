"""CPU: map_reads / map_pair -- the command lines, the argument checks of the C ABI, the binding, and the Python restatement
of the two programs against every golden the real reference wrote (tests/golden/map_*)."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_restatement as MR  # noqa: E402

BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
USAGE = {"map_reads": "map_usage_reads.txt", "map_pair": "map_usage_pair.txt"}


CASES = os.path.join(GOLDEN, "map_cases")


def golden_cases():
    return json.load(open(os.path.join(CASES, "cases.json")))


@pytest.mark.parametrize("prog", ["map_reads", "map_pair"])
def test_cli_prints_the_reference_usage(prog):
    want = open(os.path.join(GOLDEN, USAGE[prog]), "rb").read()
    r = subprocess.run([os.path.join(BIN, prog)], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == want
    r = subprocess.run([os.path.join(BIN, prog), "-h"], capture_output=True, timeout=60)
    assert r.stdout == want


def test_map_entry_points_validate_before_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p()
    good = dict(k=31, seed_kmers=5, min_read_len=250, second_alignment=1, min_identity=0.97)
    for bad in (dict(k=0), dict(k=32), dict(seed_kmers=0), dict(min_read_len=-1), dict(second_alignment=2),
                dict(min_identity=float("nan"))):
        p = capi.MapParams(**dict(good, **bad))
        assert L.dbgk_map_create(ctypes.byref(p), 0, ctypes.byref(h)) == capi.ERR_ARG, bad
    p = capi.MapParams(**good)
    assert L.dbgk_map_create(None, 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_map_create(ctypes.byref(p), -1, ctypes.byref(h)) == capi.ERR_ARG
    off = (ctypes.c_uint64 * 2)(0, 4)
    hits = (ctypes.c_int32 * 16)()
    assert L.dbgk_map_set_contigs(None, b"ACGT", off, 1) == capi.ERR_ARG
    assert L.dbgk_map_reads(None, b"ACGT", off, 1, hits) == capi.ERR_ARG
    assert L.dbgk_map_set_ramp(None, 8) == capi.ERR_ARG
    assert L.dbgk_map_batch_stats(None, None) == capi.ERR_ARG
    assert L.dbgk_map_destroy(None) == capi.ERR_ARG


def test_binding_covers_the_map_section():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in ("dbgk_map_create", "dbgk_map_destroy", "dbgk_map_set_contigs", "dbgk_map_set_ramp", "dbgk_map_reads",
              "dbgk_map_batch_stats"):
        assert n in names and hasattr(capi.lib(), n)
    assert capi.MAP_HIT_DTYPE.itemsize == 32 and ctypes.sizeof(capi.MapParams) == 24
    assert ctypes.sizeof(capi.MapStats) == 5 * 8 + 2 * 8
    assert capi.lib().dbgk_abi_version() == 7
    assert hasattr(capi.Mapper, "__enter__") and hasattr(capi.Mapper, "__exit__")


def test_no_mapper_without_gpu(tmp_path):
    """no device: the binding raises and the programs exit non-zero with a message, nothing falls back to the host"""
    from dbg_assembly_amd import capi
    if capi.lib().dbgk_device_count() > 0:
        return
    with pytest.raises(capi.DbgkError) as e:
        capi.Mapper()
    assert e.value.status == capi.ERR_HIP
    for f in ("contigs.fa", "short.lib", "short.fa"):
        shutil.copy(os.path.join(CASES, f), tmp_path / f)
    r = subprocess.run([os.path.join(BIN, "map_reads"), "-o", str(tmp_path / "o"), "contigs.fa", "short.lib"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "dbgk_map_create failed" in r.stderr


def test_identity_restatement_is_float_arithmetic():
    # what `float id = 1.0 - (float)mis / len; id < 0.97; cout << id * 100` gives when compiled with g++ -O2.  9 in 300 is the
    # telling one: (float)9 / 300 rounds down, so the float identity lands above the double 0.97 and the read is accepted
    for mis, length, ok, text in ((8, 267, True, "97.0037"), (9, 300, True, "97"), (9, 299, False, "96.99"), (0, 36, True, "100"),
                                  (10, 333, False, "96.997"), (3, 100, True, "97")):
        assert MR.accepted(mis, length, 0.97) == ok and MR.percent(mis, length) == text, (mis, length)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_golden(case):
    want = MR.expected_outputs(CASES, case)
    got = MR.run_case(CASES, case)
    assert sorted(got) == sorted(want)
    for f in sorted(want):
        assert got[f] == want[f], f


def test_goldens_cover_what_they_are_meant_to():
    """every category the issue lists shows in the reference's own output (the generator asserts the same)"""
    seen = MR.coverage(CASES, golden_cases())
    assert not [n for n in MR.NEED if n not in seen]
    assert "ctg:tiny" not in seen                      # shorter than -l
    assert {c["args"][c["args"].index("-k") + 1] for c in golden_cases() if "-k" in c["args"]} == {"21"}
