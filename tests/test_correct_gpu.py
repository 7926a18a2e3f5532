"""GPU: correct_error_reads on the MI355X against the real reference's goldens (tests/golden/correct_*), through the
command line and through capi.Corrector, and the two routes to the table.  Each GPU step is a child process under a
time limit of its own."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_correct_cpu import EXE, GOLDEN, expected_fa, golden_cases  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "correct_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("d,case", golden_cases(), ids=lambda v: v if isinstance(v, str) else v["name"])
def test_cli_matches_golden(tmp_path, d, case):
    D = os.path.join(GOLDEN, d)
    shutil.copy(os.path.join(D, case["reads"]), tmp_path / case["reads"])
    (tmp_path / "reads.lib").write_text("\t%s \n\n" % (tmp_path / case["reads"]))
    r = subprocess.run([EXE] + case["args"] + [os.path.join(D, "table.cz"), str(tmp_path / "reads.lib")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = gzip.open(tmp_path / (case["reads"] + ".correct.fa.gz"), "rb").read()
    assert got == expected_fa(d, case)
    assert (tmp_path / (case["reads"] + ".correct.stat")).read_text() == open(os.path.join(D, case["name"] + ".correct.stat")).read()
    assert r.stderr.count("node_vec_pos exceed Max_node_in_BB_tree") == case["node_limit_hits"]
    assert "Kmer_hifreq_num   %d\n" % case["hifreq"] in r.stderr


@pytest.mark.gpu
def test_capi_goldens_and_overflow_kernel():
    res = run_step("capi_goldens", 600)
    print(res)
    assert res["correct_k9_dense/n4000"]["by_overflow"] > 0   # the dense table's wide trees leave LDS
    assert all(v["by_classify"] > 0 for k, v in res.items() if "k13/default" in k)


@pytest.mark.gpu
def test_kfreq_route_equals_file_route_k17():
    res = run_step("routes", 900)
    print(res)
    assert res["by_correct"] > 0 and res["tree"] > 0 and res["one_base"] > 0
