"""GPU: map_reads / map_pair on the MI355X against the real reference's goldens (tests/golden/map_*), through the command
lines and through capi.Mapper, and one larger job against the restatement.  Each GPU step is a child process under a time
limit of its own."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_restatement as MR  # noqa: E402
from test_map_cpu import BIN, CASES, golden_cases  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "map_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_cli_matches_golden(tmp_path, case):
    D = CASES
    work = tmp_path / "in"
    work.mkdir()
    for f in os.listdir(D):
        if os.path.isfile(os.path.join(D, f)):
            shutil.copy(os.path.join(D, f), work / f)
    out = tmp_path / "out" / "dir"          # -o is created when missing
    (tmp_path / "out").mkdir()
    r = subprocess.run([os.path.join(BIN, case["program"])] + case["args"] + ["-o", str(out), case["contigs"], case["lib"]],
                       cwd=work, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = MR.expected_outputs(CASES, case)
    got = {}
    for f in os.listdir(out):
        data = open(out / f, "rb").read()
        got[f] = (gzip.decompress(data) if f.endswith(".gz") else data).decode("latin-1")
    lib_out = "%s.%s.2ctg.lib" % (case["lib"], case["program"])
    got[lib_out] = (work / lib_out).read_text().replace(str(out) + "/", "OUT/")
    assert sorted(got) == sorted(want)
    for f in sorted(want):
        assert got[f] == want[f], f


@pytest.mark.gpu
def test_capi_goldens_and_both_paths():
    res = run_step("capi_goldens", 900)
    print(res)
    st = res["reads_default"]
    assert st["by_lds"] > 0 and st["by_long"] > 0          # reads of up to 1024 bases out of LDS, longer ones out of global memory
    assert res["reads_short"]["skipped"] > 0         # reads of k + s - 1 bases
    assert all(v["windows_probed"] > 0 for v in res.values())


@pytest.mark.gpu
def test_large_job_sample_and_batch_independence():
    res = run_step("large", 1500)
    print(res)
    # 500 contigs of 5 000 bases drawn from 3 Mb cover 1 - exp(-2.5 / 3) = 57 % of the genome, and where two of them overlap the
    # k-mers are no longer unique: well over a quarter of the reads must still map, and some of them twice
    assert res["mapped"] > res["reads"] // 4 and res["second"] > 0


def edge_cases():
    from test_map_edges_cpu import edge_golden_cases
    return edge_golden_cases()


@pytest.mark.gpu
def test_edges_match_restatement_field_for_field():
    """the crafted scenarios of tests/map_edge_cases.py: every category compared, at all three ramps, out of LDS and out of
    global memory"""
    import map_edge_cases as E
    res = run_step("edges", 300)
    print(res)
    assert sorted(res["categories"]) == sorted(E.CATEGORIES + ["grid"])
    assert all(v > 0 for v in res["categories"].values())
    assert res["ramps"] == [1, 4, 64] and res["by_lds"] > 0 and res["by_long"] > 0 and res["skipped"] > 0
    assert res["categories"]["grid"] == 4 * 32 * res["n_cu"] + 5
    assert res["golden_cases"] == len(edge_cases()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: c["name"])
def test_cli_matches_edge_golden(tmp_path, case):
    """bin/map_reads and bin/map_pair on the reference-written cases of tests/golden/map_edge_cases"""
    from test_map_edges_cpu import EDGE_CASES, edge_expected
    work = tmp_path / "in"
    work.mkdir()
    for f in [case["contigs"], case["lib"]] + MR.read_lib_file(os.path.join(EDGE_CASES, case["lib"])):
        shutil.copy(os.path.join(EDGE_CASES, f), work / f)
    out = tmp_path / "out"
    r = subprocess.run([os.path.join(BIN, case["program"])] + case["args"] + ["-o", str(out), case["contigs"], case["lib"]],
                       cwd=work, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = edge_expected(case)
    got = {}
    for f in os.listdir(out):
        data = open(out / f, "rb").read()
        got[f] = (gzip.decompress(data) if f.endswith(".gz") else data).decode("latin-1")
    lib_out = "%s.%s.2ctg.lib" % (case["lib"], case["program"])
    got[lib_out] = (work / lib_out).read_text().replace(str(out) + "/", "OUT/")
    assert sorted(got) == sorted(want)
    for f in sorted(want):
        assert got[f] == want[f], f
