"""GPU: the cleaner's output stage and the hand-off of its compact batch to the next stage.  Crafted batches through compact_from
against the numpy restatement (tests/clean_compact_restatement.py), both planes and all eight counters; Cleaner.lowqual /
Cleaner.adapter + compact against lines 2 and 4 and the stat numbers the real reference wrote, and against Cleaner.trim_* on the
pinned edge scenarios; the _device calls against the host-input calls; the chain from one upload through both cleaning stages to a
k = 17 frequency table, the corrector and a finalized k = 31 graph against today's host route.  Each GPU step is a child process
under a time limit of its own (tests/clean_compact_gpu_steps.py); the limits only end a stuck step.

dbgk_clean_adapter takes no qualities, so after Cleaner.adapter the compact batch has no quality plane: line 4 of the adapter
goldens is checked on the batch of adapter_device, whose records and base plane are first held to those of Cleaner.adapter."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_edge_cases as E  # noqa: E402
import clean_restatement as CR  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "clean_compact_gpu_steps.py")
CASES = os.path.join(ROOT, "tests", "golden", "clean_cases")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_crafted_batches_equal_the_restatement_on_both_planes_and_the_counters():
    res = run_step("crafted", 120)
    print(res)
    shapes = ["n1", "all_emptied", "lengths_1_100", "total_T", "total_T_plus_1", "total_T_minus_1", "total_15", "empty_run_3T_inside_a_tile",
              "empty_run_ends_on_a_tile_boundary", "empty_run_ends_one_byte_past_a_boundary", "first_and_last_empty",
              "source_and_destination_mod_4", "min_len_boundary", "min_len_0_empty_input_reads", "record_keeps_nothing"]
    shapes += ["long_read_spans_three_tiles_src%d" % a for a in range(16)]
    for tag in ("lowqual", "adapter"):
        for s in shapes:
            assert "%s/%s" % (tag, s) in res, (tag, s)
        assert res[tag + "/all_emptied"]["bases"] == 0 and res[tag + "/total_15"]["bases"] == 15
        assert sorted(res[tag + "/long_read_src_mod16"]) == list(range(16))
    assert res["lowqual/N_shift33"]["rewritten"] == 2 and res["lowqual/N_shift64"]["rewritten"] == 2
    assert res["lowqual/clean_reads_of_8_with_5_empty"] == 3 and res["adapter/clean_reads_of_8_with_5_empty"] == 8
    assert res["outside"] == {"lowqual": 4, "adapter": 4}


@pytest.mark.gpu
def test_goldens_compact_equals_lines_2_and_4_and_the_stat_of_the_reference():
    res = run_step("goldens", 120)
    print(res)
    assert sorted(res) == sorted(c["name"] for c in CR.golden_cases(CASES))
    assert res["adapter_norecords"]["reads"] == 0 and res["lowqual_norecords"]["reads"] == 0
    assert any(v["trimmed_reads"] > 0 and v["short_reads"] > 0 for k, v in res.items() if k.startswith("adapter"))
    assert any(v["trimmed_reads"] > 0 and v["short_reads"] > 0 for k, v in res.items() if k.startswith("lowqual"))


@pytest.mark.gpu
def test_edge_scenarios_compact_equals_what_trim_makes_of_them():
    res = run_step("edges", 180)
    print(res)
    assert sorted(res) == sorted(s.name for s in E.scenarios() if E.pinned(s))
    assert res["N_shift64"]["trimmed_reads"] == 3 and res["chunks"]["reads"] == 5 * E.GROUP + 3


@pytest.mark.gpu
def test_device_input_equals_host_input_and_is_left_unchanged():
    res = run_step("device_input", 120)
    print(res)
    assert res["adapter"]["reads"] == res["lowqual"]["reads"] == 3000


@pytest.mark.gpu
def test_one_upload_from_raw_reads_to_the_table_the_corrector_and_the_graph():
    res = run_step("chain", 300)
    print(res)
    assert res["emptied_by_lowqual"] > 0 and res["emptied_by_adapter"] > 0 and res["kept"] > 0 and res["cut_and_kept"] > 0
    assert res["direct"] == res["partition"]


@pytest.mark.gpu
def test_cleaners_are_reused_at_once_and_a_compact_batch_goes_into_two_handles():
    res = run_step("reuse", 180)
    print(res)
    assert res["reads"] == 4000


@pytest.mark.gpu
def test_the_error_returns():
    from dbg_assembly_amd import capi
    res = run_step("states", 120)
    print(res)
    want = {"compact_before_any_batch": capi.ERR_STATE, "device_before_any_compact": capi.ERR_STATE, "push_before_any_compact": capi.ERR_STATE,
            "quality_plane_of_a_batch_without_one": capi.ERR_ARG, "results_with_no_pointer": capi.OK,
            "own_bases_as_adapter_input": capi.ERR_ARG, "own_quals_as_adapter_quals": capi.ERR_ARG, "own_planes_as_lowqual_input": capi.ERR_ARG,
            "misaligned_plane": capi.ERR_ARG, "negative_min_len": capi.ERR_ARG, "compact_after_the_refusals": capi.OK,
            "push_into_a_finalized_handle": capi.ERR_STATE}
    assert res == want
