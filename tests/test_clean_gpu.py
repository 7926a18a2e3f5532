"""GPU: clean_adapter / clean_lowqual on the MI355X against the real reference's goldens (tests/golden/clean_*), through the
command lines and through capi.Cleaner, and one larger job against the restatement in which every read is compared.  Each GPU
step is a child process under a time limit of its own."""
import gzip
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_restatement as CR  # noqa: E402
from test_clean_cpu import BIN, CASES, golden_cases  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "clean_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_cli_matches_golden(tmp_path, case):
    r = subprocess.run([os.path.join(BIN, case["program"])] + case["args"] + [case["input"], str(tmp_path / "out.gz"), str(tmp_path / "out.stat")],
                       cwd=CASES, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = CR.expected_outputs(CASES, case)
    assert gzip.decompress((tmp_path / "out.gz").read_bytes()).decode("latin-1") == want["out"]
    assert (tmp_path / "out.stat").read_bytes().decode("latin-1") == want["stat"]


@pytest.mark.gpu
def test_capi_goldens_and_both_forms():
    res = run_step("capi_goldens", 600)
    print(res)
    st = res["adapter_contaminants"]
    assert st["by_lds"] > 0 and st["by_global"] > 0       # reads of up to 1024 bases out of LDS, the 1500- and 2000-base reads out of global memory
    assert res["large_set"]["by_lds"] == 0 and res["large_set"]["by_global"] == res["large_set"]["reads"]
    assert all(v["cells"] > 0 for k, v in res.items() if k.startswith("adapter_") and "norecords" not in k)
    assert res["adapter_norecords"]["reads"] == 0


@pytest.mark.gpu
def test_large_job_every_read_and_batch_independence():
    res = run_step("large", 1500)
    print(res)
    assert res["reads"] >= 100000 and res["by_lds"] > 0 and res["by_global"] > 0
    # one read in ten carries a contaminant prefix of 6 bases or more with 5 % substitutions; those of 10 clean bases or more reach the
    # cutoff of 10 -- well over half of them -- and random sequence reaches it only rarely
    assert res["reads"] // 20 < res["hits"] < res["reads"] // 5
    assert 0 < res["trimmed"] < res["reads"]
