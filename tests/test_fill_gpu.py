"""GPU: link_contig on the MI355X against the real reference's goldens (tests/golden/fill_cases), through the command line and
through capi.GapFiller, the mapper's hits against the 2ctg text, map_reads -> link_contig end to end, and a larger job against the
restatement.  Each GPU step is a child process under a time limit of its own."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fill_restatement as FR  # noqa: E402
import link_restatement as LR  # noqa: E402
from test_fill_cpu import BIN, CASES, golden_cases  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "fill_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_cli_matches_golden(tmp_path, case):
    work = tmp_path / "in"
    LR.unpack_inputs(CASES, case, work)
    r = subprocess.run([os.path.join(BIN, "link_contig")] + case["args"] + ["-o", case["prefix"], case["contigs"], case["lib"]],
                       cwd=work, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = LR.expected_outputs(CASES, case)
    got = {f: open(work / f, encoding="latin-1").read() for f in os.listdir(work) if f.startswith(case["prefix"] + ".")}
    got["stderr.txt"] = LR.strip_run_time(r.stderr.decode("latin-1"))
    assert len(got) == 7
    FR.compare_outputs(case, got, want)


@pytest.mark.gpu
def test_gap_filler_equals_the_restatement_on_every_fixture():
    res = run_step("cases", 600)
    print(res)
    assert len(res) == 4 and all(v["filled"] > 0 for v in res.values())


@pytest.mark.gpu
def test_map_reads_to_link_contig_returns_the_source_sequence():
    res = run_step("pipeline", 900)
    print(res)
    assert res["length"] == 9000 and res["two_contig_reads"] >= 20


@pytest.mark.gpu
def test_large_job_equals_the_restatement():
    res = run_step("large", 1500)
    print(res)
    assert res["gaps"] > 3000 and res["filled"] > 1000 and res["cut"] > 1000 and res["max_span"] > 2000


@pytest.mark.gpu
def test_emit_equals_the_restatement():
    res = run_step("emit", 600)
    print(res)
    assert res["bytes"] > (1 << 21)
