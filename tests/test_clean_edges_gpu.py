"""GPU: k_clean_adapter (both forms) and k_clean_lowqual on the edge scenarios of tests/clean_edge_cases.py -- per read every field
of the hit or block (error_sum as a bit pattern) against the restatement, and the batch counters against what the construction
says; one handle through the branches of the host side; and the two programs over one edge FASTQ each against the bytes the
real reference wrote (tests/golden/clean_edges).  Each GPU step is a child process under a time limit of its own; the limits
only end a stuck step."""
import gzip
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_edge_cases as E  # noqa: E402
import clean_restatement as CR  # noqa: E402
from test_clean_cpu import BIN  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "clean_edges_gpu_steps.py")
EDGES = os.path.join(ROOT, "tests", "golden", "clean_edges")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_edges_adapter_every_field_and_counter_in_both_forms():
    res = run_step("edges_adapter", 300)
    print(res)
    assert sorted(res) == sorted(s.name for s in E.adapter_scenarios())
    assert (res["slice_edge"]["by_lds"], res["slice_edge"]["by_global"]) == (1, 2)
    for t in E.SET_SIZES:
        st = res["set_size_%d" % t]
        assert (st["by_lds"], st["by_global"], st["hits"]) == ((3, 0, 2) if t <= E.SET_BYTES else (0, 3, 2))
    for s in E.adapter_scenarios():          # each tie scenario in the LDS form and in the global-memory form
        if s.name.startswith("tie_") and s.name.endswith("_lds"):
            a, b = res[s.name], res[s.name[:-3] + "global"]
            assert a["by_global"] == b["by_lds"] == 0 and a["by_lds"] == b["by_global"] == a["hits"] == b["hits"] == len(s.reads)
            assert a["cells"] == b["cells"]  # every read is hit by the first contaminant: the ones that fill the set are never aligned


@pytest.mark.gpu
def test_edges_lowqual_blocks_bit_for_bit():
    res = run_step("edges_lowqual", 300)
    print(res)
    assert sorted(res) == sorted(s.name for s in E.lowqual_scenarios())
    for name in E.EQUAL_RATE:
        assert res[name]["trimmed"] == sum(e["trimmed"] for e in E.scenario(name).expect)
    assert res["chunks"]["reads"] == 5 * E.GROUP + 3 and res["groups_513"]["trimmed"] == len(E.TELLING)


@pytest.mark.gpu
def test_edges_host_one_handle_through_every_branch():
    res = run_step("edges_host", 300)
    print(res)
    assert res["big"]["reads"] == 1200 and res["tie_t1_global"]["by_global"] == res["tie_t1_lds"]["by_lds"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["staging", "chunks"])
def test_cli_matches_edge_golden(tmp_path, name):
    """clean_adapter over the staging scenario (every staged length at every byte offset of the batch) and clean_lowqual over the
    chunk scenario, against what the reference's programs wrote"""
    case = next(c for c in json.load(open(os.path.join(EDGES, "cases.json"))) if c["name"] == name)
    r = subprocess.run([os.path.join(BIN, case["program"])] + case["args"] + [case["input"], str(tmp_path / "out.gz"), str(tmp_path / "out.stat")],
                       cwd=EDGES, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = CR.expected_outputs(EDGES, case)
    assert gzip.decompress((tmp_path / "out.gz").read_bytes()).decode("latin-1") == want["out"]
    assert (tmp_path / "out.stat").read_bytes().decode("latin-1") == want["stat"]
