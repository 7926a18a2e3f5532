"""CPU: the writer of <lib>.kmer.freq.stat (dbg_assembly_amd/host/kmer_spectrum.h) rebuilds the three spectra the reference
ships byte for byte from their species column alone (tests/golden/kmerfreq_stat/*.json: the non-zero rows and the
SHA-256 of the whole 65542-line file), through tests/kmer_spectrum_test.cpp -- built plain and with
-fsanitize=address,undefined -- and through the Python restatement the GPU tests use.  Also the C ABI's argument checks
and the binding of the two device spectra."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spectrum_restatement as SR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "kmerfreq_stat")
NAMES = ["clean", "raw", "corrected"]


def fixture_of(name):
    return json.load(open(os.path.join(GOLDEN, name + ".json")))


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def exe(tmp_path_factory, request):
    out = str(tmp_path_factory.mktemp("spectrum") / "kmer_spectrum_test")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "asan_ubsan" else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "dbg_assembly_amd", "host"),
                    os.path.join(ROOT, "tests", "kmer_spectrum_test.cpp"), "-o", out] + extra, check=True)
    return out


def test_fixtures_are_the_references_three_files():
    rows = {n: fixture_of(n) for n in NAMES}
    assert [len(rows[n]["rows"]) for n in NAMES] == [567, 567, 578]
    assert [rows[n]["rows"][-1][0] for n in NAMES] == [3975, 3975, 4055]
    for g in rows.values():
        assert (g["k"], g["max_freq"], g["lines"], g["space"]) == (17, 65535, 65542, 4 ** 17)
        assert g["species"] == sum(s for _, s in g["rows"]) and g["individuals"] == sum(f * s for f, s in g["rows"])


@pytest.mark.parametrize("name", NAMES)
def test_writer_rebuilds_the_reference_file_byte_for_byte(exe, tmp_path, name):
    g = fixture_of(name)
    hist = tmp_path / "hist.txt"
    hist.write_text("%d %d %d %d\n" % (g["k"], g["max_freq"], g["individuals"], len(g["rows"]))
                    + "".join("%d %d\n" % (f, s) for f, s in g["rows"]))
    r = subprocess.run([exe, "write", str(hist)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == b""   # nothing from a sanitizer
    assert len(r.stdout) == g["bytes"]
    assert hashlib.sha256(r.stdout).hexdigest() == g["sha256"]
    head = r.stdout.decode().split("\n")[:5]
    assert head[4] == "#Theoretic space of Kmer species: %d  occupied ratio: %s" % (g["space"], g["occupied_ratio"])


def test_writer_rules_remainder_empty_and_k1(exe):
    r = subprocess.run([exe, "self"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]


@pytest.mark.parametrize("name", NAMES)
def test_python_restatement_rebuilds_the_reference_file(name):
    g = fixture_of(name)
    text = SR.spectrum_text(g["k"], g["max_freq"], dict(map(tuple, g["rows"])), g["individuals"]).encode()
    assert len(text) == g["bytes"] and hashlib.sha256(text).hexdigest() == g["sha256"]


def test_python_restatement_follows_the_writers_own_rules():
    t = SR.spectrum_text(2, 3, [99, 3, 1, 1], 10).split("\n")
    assert t[7:10] == ["1\t3\t0.6\t0.6\t3\t0.3\t0.3", "2\t1\t0.2\t0.8\t2\t0.2\t0.5", "3\t1\t0.2\t1\t5\t0.5\t1"]
    assert SR.spectrum_text(3, 2, [0, 0, 0], 0).split("\n")[4:] == [
        "#Theoretic space of Kmer species: 64  occupied ratio: 0", "", SR.COLUMNS[:-1], "1\t0\t0\t0\t0\t0\t0", "2\t0\t0\t0\t0\t0\t0", ""]


def test_binding_covers_the_spectrum_entry_points():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in ("dbgk_kfreq_spectrum", "dbgk_kfreq_spectrum_ms", "dbgk_comm_kfreq_spectrum", "dbgk_corr_mutation_scan",
              "dbgk_corr_mutation_scan_ms"):
        assert n in names and hasattr(capi.lib(), n)
    for cls, m in ((capi.Graph, "kfreq_spectrum"), (capi.Comm, "kfreq_spectrum"), (capi.Corrector, "mutation_scan")):
        assert callable(getattr(cls, m))
    assert capi.lib().dbgk_abi_version() == 7


def test_null_arguments_are_refused_before_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    hist = (ctypes.c_uint64 * 256)()
    assert L.dbgk_kfreq_spectrum(None, 0, 0, hist) == capi.ERR_ARG
    assert L.dbgk_comm_kfreq_spectrum(None, hist) == capi.ERR_ARG
    assert L.dbgk_corr_mutation_scan(None, None, None, 0, 1, hist) == capi.ERR_ARG
    assert L.dbgk_kfreq_spectrum_ms(None, None) == capi.ERR_ARG and L.dbgk_corr_mutation_scan_ms(None, None) == capi.ERR_ARG
