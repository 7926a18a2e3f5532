"""GPU: link_supertig on the MI355X against the real reference's goldens (tests/golden/super_cases), through the command line and
through capi.SuperLinker, the mapper's hits against the 2ctg text, map_reads -> link_supertig end to end, and a random job sized
for the kernels against the restatement.  Each GPU step is a child process under a time limit of its own."""
import gzip
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import link_restatement as LR  # noqa: E402
import super_restatement as SR  # noqa: E402
from test_super_cpu import BIN, CASES, golden_cases  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "super_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_cli_matches_golden(tmp_path, case):
    work = tmp_path / "in"
    LR.unpack_inputs(CASES, case, work)
    r = subprocess.run([os.path.join(BIN, "link_supertig")] + case["args"] + ["-o", case["prefix"], case["contigs"], case["lib"]],
                       cwd=work, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = LR.expected_outputs(CASES, case)
    got = {f: open(work / f, encoding="latin-1").read() for f in os.listdir(work) if f.startswith(case["prefix"] + ".")}
    got["stderr.txt"] = LR.strip_run_time(r.stderr.decode("latin-1"))
    assert len(got) == 8
    SR.compare_outputs(case, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["short", "missing"])
def test_cli_names_the_read_that_has_no_slice(tmp_path, what):
    """a spanning read that is too short for its slice, or in no reads file: exit 1 with the read and both contigs named"""
    case = next(c for c in golden_cases() if c["name"] == "n1")
    work = tmp_path / "c"
    LR.unpack_inputs(CASES, case, work)
    f = work / "part1.map_reads.2ctg.gz.reads.fa.gz"
    lines = gzip.decompress(f.read_bytes()).decode("latin-1").split("\n")
    assert lines[0] == ">read_1"                       # the first record spans ctg_1 and ctg_3, a junction of the layout
    lines[0:2] = [">read_1", lines[1][:100]] if what == "short" else []
    f.write_bytes(gzip.compress("\n".join(lines).encode("latin-1")))
    r = subprocess.run([os.path.join(BIN, "link_supertig")] + case["args"] + ["-o", "x", case["contigs"], case["lib"]], cwd=work,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stderr[-3000:]
    assert "link_supertig: read read_1 that spans ctg_1 and ctg_3 is missing from the .reads.fa.gz files or too short" in r.stderr
    assert "dbgk_super_resolve failed" in r.stderr and "Program finished" not in r.stderr


@pytest.mark.gpu
def test_super_linker_equals_the_restatement_on_every_fixture():
    res = run_step("cases", 600)
    print(res)
    assert len(res) == 4 and all(v["lines"] > 0 and v["slices"] > v["lines"] for v in res.values())


@pytest.mark.gpu
def test_map_reads_to_link_supertig_returns_the_source_sequence():
    res = run_step("pipeline", 600)
    print(res)
    assert res["length"] == 12000 - 170 + sum(res["gaps"]) and res["two_contig_reads"] >= 30


@pytest.mark.gpu
def test_random_job_equals_the_restatement():
    res = run_step("random", 600)
    print(res)
    assert res["records"] > 3000 and res["junctions"] > 150
