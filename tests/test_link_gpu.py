"""GPU: link_scaffold on the MI355X against the real reference's goldens (tests/golden/link_cases), through the command line and
through capi.Scaffolder, the mapper's hits against the 2ctg text, and larger jobs against the restatement.  Each GPU step is a
child process under a time limit of its own."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import link_restatement as LR  # noqa: E402
from test_link_cpu import BIN, CASES, compare_outputs, golden_cases  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "link_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in golden_cases() if "contigs" in c], ids=lambda c: c["name"])
def test_cli_matches_golden(tmp_path, case):
    work = tmp_path / "in"
    LR.unpack_inputs(CASES, case, work)
    r = subprocess.run([os.path.join(BIN, "link_scaffold")] + case["args"] + ["-o", case["prefix"], case["contigs"], case["lib"]],
                       cwd=work, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = LR.expected_outputs(CASES, case)
    got = {f: open(work / f, encoding="latin-1").read() for f in os.listdir(work) if f.startswith(case["prefix"] + ".")}
    got["stderr.txt"] = LR.strip_run_time(r.stderr.decode("latin-1"))
    assert len(got) == 7
    compare_outputs(case, got, want)


@pytest.mark.gpu
def test_scaffolder_reproduces_the_ecoli_runs():
    res = run_step("ecoli", 600)
    print(res)
    assert res["ecoli_insert400"]["records"] == 6479 and res["ecoli_insert800"]["records"] == 769


@pytest.mark.gpu
def test_mapper_hits_give_the_table_of_the_2ctg_text():
    res = run_step("hits", 900)
    print(res)
    assert all(v["two_contig_pairs"] > 0 and v["pairs"] > v["two_contig_pairs"] for v in res.values())


@pytest.mark.gpu
def test_large_job_equals_the_restatement():
    res = run_step("large", 1500)
    print(res)
    assert res["kept"] > res["records"] // 4 and res["scaffolds"] > 1000 and res["repeat_nodes"] > 0


@pytest.mark.gpu
def test_emit_equals_the_restatement():
    res = run_step("emit", 600)
    print(res)
    assert res["bytes"] > (1 << 21)
