"""GPU: the PAIR stage (csrc/dbgk_pair.h) and the mapper's device entry.  Crafted batches through Pairer.split against the numpy
restatement (tests/pair_restatement.py) byte for byte -- whole 16-byte vectors of every plane with the zero pad, offsets, source
ids, counters -- with and without quality planes; device input that is a sub-range of larger buffers; the reference's -j 1 files
(tests/golden/pair_cases) from two correctors' compact batches and from bin/correct_error_reads -j 1 as a program; the hand-offs to
a graph handle and to the mapper.  Each GPU step is a child process under a time limit of its own (tests/pair_gpu_steps.py); the
limits only end a stuck step."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_restatement as PR  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "pair_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_crafted_batches_equal_the_restatement_byte_for_byte():
    res = run_step("crafted", 180)
    print(res)
    shapes = ["n0", "n1_both", "n1_only1", "n1_only2", "n1_neither", "all_pairs_kept", "none_kept", "all_single_from_mate1",
              "all_single_from_mate2", "lengths_1_100", "long_read_is_mate2_of_a_kept_pair", "dropped_run_3T_inside_a_tile",
              "dropped_run_3T_at_a_tile_boundary", "single_run_3T_between_kept_pairs", "first_and_last_dropped", "first_and_last_kept"]
    shapes += ["classes_cycle_n%d" % n for n in (63, 64, 65, 255, 256, 257)]
    shapes += ["%s_total_%s" % (w, t) for w in ("pair", "single") for t in ("15", "16", "17", "T_minus_1", "T", "T_plus_1")]
    for s in shapes:
        assert s in res, s
    zero = {"pair_reads": 0, "pair_bases": 0, "single_reads": 0, "single_bases": 0}
    assert res["n0"] == zero and res["n1_neither"] == zero and res["none_kept"] == zero
    assert res["n1_both"] == dict(zero, pair_reads=2, pair_bases=78) and res["n1_only1"] == dict(zero, single_reads=1, single_bases=37)
    assert res["n1_only2"] == dict(zero, single_reads=1, single_bases=41)
    assert res["all_single_from_mate1"]["single_reads"] == res["all_single_from_mate2"]["single_reads"] == 700
    assert res["all_pairs_kept"]["single_reads"] == 0 and res["all_pairs_kept"]["pair_bases"] == 30000
    assert res["classes_cycle_n257"] == dict(pair_reads=2 * 65, single_reads=128, pair_bases=res["classes_cycle_n257"]["pair_bases"],
                                             single_bases=res["classes_cycle_n257"]["single_bases"])
    assert res["lengths_1_100_residues"] == "all"


@pytest.mark.gpu
def test_the_rank_crosses_many_workgroups():
    res = run_step("many", 120)
    print(res)
    assert res["n70000"]["pair_reads"] > 80000 and res["n70000"]["single_reads"] > 20000


@pytest.mark.gpu
def test_device_input_reads_nothing_outside_its_range():
    res = run_step("subrange", 120)
    print(res)
    assert len(res) == 3 and all(v["pair_reads"] > 0 and v["single_reads"] > 0 for v in res.values())


@pytest.mark.gpu
def test_two_compact_batches_split_on_the_device_equal_the_reference_files():
    res = run_step("goldens", 180)
    print(res)
    for name, (_, _, (both, only1, only2, _)) in PR.CASES.items():
        assert res[name]["pair_reads"] == 2 * both and res[name]["single_reads"] == only1 + only2, name


@pytest.mark.gpu
def test_correct_error_reads_j1_writes_the_reference_files():
    """fails without the PAIR stage: the program refused -j 1"""
    res = run_step("cli", 300)
    print(res)
    assert sorted(res) == sorted(list(PR.CASES) + ["different_record_counts"]) and res["different_record_counts"] == 1
    assert res["default"] == ["678", "95797", "68", "10593"]


@pytest.mark.gpu
def test_both_outputs_pushed_into_a_graph_equal_the_same_reads_from_the_host():
    res = run_step("graph", 240)
    print(res)
    assert res["direct"] == res["partition"] and res["direct"]["nodes"] > 1000


@pytest.mark.gpu
def test_map_device_on_the_pair_batch_equals_map_on_its_host_copy():
    from dbg_assembly_amd import capi
    res = run_step("mapper", 120)
    print(res)
    assert res["with_a_long_read"]["by_long"] > 0 and res["reads"]["by_long"] == 0
    assert res["max_len_too_small"] == capi.ERR_ARG


@pytest.mark.gpu
def test_a_pairer_is_reused_at_once_and_regrows():
    res = run_step("reuse", 240)
    print(res)
    assert res["reads"] > 15000


@pytest.mark.gpu
def test_the_error_returns():
    from dbg_assembly_amd import capi
    res = run_step("states", 120)
    print(res)
    want = {"results_before_a_split": capi.ERR_STATE, "device_before_a_split": capi.ERR_STATE, "push_before_a_split": capi.ERR_STATE,
            "which_out_of_range": capi.ERR_ARG, "misaligned_plane": capi.ERR_ARG, "own_output_as_input": capi.ERR_ARG,
            "qualities_for_one_mate_only": capi.ERR_ARG, "offsets_that_do_not_start_at_0": capi.ERR_ARG,
            "results_after_a_refused_split": capi.OK, "quality_plane_of_an_output_without_one": capi.ERR_ARG,
            "results_with_no_pointer": capi.OK, "push_into_a_finalized_handle": capi.ERR_STATE}
    assert res == want
