"""GPU: the LINK and FILL kernels on the edge scenarios of tests/scaffold_edge_cases.py -- k_fill_consensus beyond 64 columns and
64 spanning reads on both strands, every column tie, the host path met in the last unit of the last round, fill_run_end around the
powers of two, the bad-slice rule at the end of the read, more work units than waves, the gap filter of every class at both ends,
the 1023 cap across batches, a gap sum beyond 2^31, first-seen order and the drop conditions for mapper hits -- against the
restatements, and the two programs over the golden subset against the bytes the real reference wrote
(tests/golden/scaffold_edges).  tests/test_scaffold_edges_cpu.py shows that the scenarios sit where they claim.  Each GPU step is a
child process under a time limit of its own; the limits only end a stuck step."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scaffold_edge_cases as E  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "scaffold_edges_gpu_steps.py")
EDGES = os.path.join(ROOT, "tests", "golden", "scaffold_edges")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_fill_consensus_at_every_width_span_and_tie():
    res = run_step("fill_consensus", 120)
    print(res)
    assert res["widths_x_spans"]["filled"] == 64 == len(E.WIDTHS) * len(E.SPANS) and res["widths_x_spans"]["records"] == 5312
    assert res["column_ties"] == {"filled": 2, "columns": 260}
    assert res["host_path_late"] == {"filled": 3, "host_path": [1, 1, 0]}


@pytest.mark.gpu
def test_fill_gapstat_run_ends():
    res = run_step("fill_gapstat", 120)
    print(res)
    assert sorted(res) == ["gapstat_last_single", "gapstat_runs"]
    assert all(v["max_span"] == 1025 and v["filled"] > 20 for v in res.values())
    assert res["gapstat_last_single"]["pairs"] == res["gapstat_runs"]["pairs"] == 55


@pytest.mark.gpu
def test_fill_slices_at_the_end_of_the_read():
    res = run_step("fill_slices", 120)
    print(res)
    assert res["refused"] == [k % at for at in E.BAD_AT for k in ("short_%d", "negative_%d")] and len(res["refused"]) == 8
    assert res["resolved"] == {"exact": 2, "modes_not_positive": 0}


@pytest.mark.gpu
def test_fill_more_units_than_waves():
    res = run_step("fill_stride", 120)
    print(res)
    assert res["filled"] == res["units"] == 40000 > res["waves"]


@pytest.mark.gpu
def test_fill_hits_filter():
    res = run_step("fill_hits", 120)
    print(res)
    assert res == {"reads": 40, "pooled": 20, "filled": 5}


@pytest.mark.gpu
def test_link_edges():
    res = run_step("link_edges", 120)
    print(res)
    for m, I in E.FILTER_JOBS:
        assert res["filter_edges_m%d_i%d" % (m, I)] == {"records": 16, "kept": 8, "links": 8, "max_freq": 2, "at_cap": 0,
                                                       "max_size": I - I // 2 + 1}
    cap = res["cap_across_batches"]
    # at the cap: the keys of 1023, 1024, 1025 and 2047 records and the large-insert key, two directed entries each (the key of
    # 1022 records stays below it)
    assert cap["max_freq"] == 1023 and cap["at_cap"] == 2 * (4 + 1) and cap["max_size"] > 2 ** 31 and cap["kept"] == cap["records"] == 9218
    assert res["first_seen_order"]["links"] == 2 * (200 + 40) and res["first_seen_order"]["max_freq"] == 2
    for m in (0, 1):
        assert res["link_hits_m%d" % m]["pairs"] == 40 and res["link_hits_m%d" % m]["kept"] == 20


@pytest.mark.gpu
def test_cli_matches_the_edge_goldens():
    res = run_step("cli_edges", 300)
    print(res)
    cases = json.load(open(os.path.join(EDGES, "cases.json")))
    assert sorted(res) == sorted(c["name"] for c in cases) and len(res) == 12
    assert sum(v == 7 for v in res.values()) == 10 and sum(v == 5 for v in res.values()) == 2
