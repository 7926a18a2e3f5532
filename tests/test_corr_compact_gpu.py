"""GPU: the corrector's output stage and the hand-off of its compact batch to a graph handle.  Crafted batches through
compact_from against the numpy restatement (tests/corr_compact_restatement.py); Corrector.correct + compact against the
sequence lines and stat numbers the real reference wrote; correct_device against correct; the chain from one upload to a
finalized k = 31 graph against the graph of today's host route.  Each GPU step is a child process under a time limit of its
own (tests/corr_compact_gpu_steps.py); the limits only end a stuck step."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import correct_edge_cases as E  # noqa: E402
from test_correct_cpu import golden_cases  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "corr_compact_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_crafted_batches_equal_the_restatement_byte_for_byte():
    res = run_step("crafted", 120)
    print(res)
    assert sorted(res) == sorted(["n1", "all_deleted", "lengths_1_100", "total_T", "total_T_plus_1", "total_T_minus_1", "total_15",
                                  "zero_run_3T_inside_a_tile", "zero_run_on_a_tile_boundary", "zero_run_one_byte_past_a_boundary",
                                  "zero_first_and_last", "long_read_spans_three_tiles_0", "long_read_spans_three_tiles_5",
                                  "trims_use_up_the_read", "source_and_destination_mod_4"])
    assert res["all_deleted"]["bases"] == 0 and res["total_15"]["bases"] == 15
    assert res["long_read_spans_three_tiles_0"]["reads"] == 5


@pytest.mark.gpu
def test_goldens_compact_equals_the_reference_sequence_lines_and_stat():
    res = run_step("goldens", 120)
    print(res)
    assert sorted(res) == sorted("%s/%s" % (d, c["name"]) for d, c in golden_cases())
    assert res["correct_k9_dense/n4000"]["by_overflow"] > 0 and any(v["deleted_reads"] > 0 for v in res.values())


@pytest.mark.gpu
def test_edge_scenarios_k13_and_below_compact_equals_the_reference():
    res = run_step("edges_small", 120)
    print(res)
    assert sorted(res) == sorted(s.name for s in E.scenarios() if s.pinned and s.k <= 13)
    assert res["trim_clamp"]["deleted_reads"] == 1


@pytest.mark.gpu
def test_edge_scenarios_k15_16_17_compact_equals_the_reference():
    res = run_step("edges_chunks", 120)
    print(res)
    assert sorted(res) == sorted(s.name for s in E.scenarios() if s.pinned and s.k > 13)


@pytest.mark.gpu
def test_correct_device_equals_correct_on_the_host_copy():
    print(run_step("device_input", 120))


@pytest.mark.gpu
def test_hand_off_builds_the_graph_of_the_host_route_direct_and_partition():
    res = run_step("handoff", 180)
    print(res)
    assert res["direct"]["deleted_reads"] > 0 and res["direct"]["trimmed_reads"] > 0


@pytest.mark.gpu
def test_corrector_is_reused_at_once_and_a_compact_batch_is_pushed_twice():
    print(run_step("reuse", 180))


@pytest.mark.gpu
def test_one_compact_batch_goes_into_a_graph_and_a_kfreq_handle():
    res = run_step("two_handles", 180)
    print(res)
    assert res["reads"] == 200000
