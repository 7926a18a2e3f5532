"""GPU: the DEFLATE stage (csrc/dbgk_gz.h) -- bytes to BGZF-framed gzip members.  Every crafted input (tests/deflate_cases.py) at every
level through Deflater.deflate against the plain restatement of the rules, at levels 0, 1 and 2, (tests/deflate_restatement.py, anchored to gzip and zlib
by tests/test_deflate_cpu.py) byte for byte, with gzip.decompress as the arbiter of CRC-32 and ISIZE and the counters compared;
more members than the member kernel's grid; repeated calls and a second handle; device input inside a larger buffer; stream() at
every window size; the hand-over from a text on the device to the parser.  Each GPU step is a child process under a time limit of
its own (tests/deflate_gpu_steps.py); the limits only end a stuck step.  Every test here fails without the stage: capi.Deflater
does not exist."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_cases as DC  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "deflate_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_crafted_inputs_equal_the_restatement_byte_for_byte():
    res = run_step("crafted", 180)
    names = list(DC.cases())
    assert len(names) > 690 and all(n in res for n in names)
    assert res["empty"] == {"n_members": 0, "out_bytes": 28, "stored_members": 0, "n_matches": 0}
    assert res["one_byte"] == {"n_members": 1, "out_bytes": 18 + 5 + 1 + 8 + 28, "stored_members": 1, "n_matches": 0}
    assert res["random_bytes"] == {"n_members": 2, "out_bytes": DC.PIECE + 1000 + 2 * 31 + 28, "stored_members": 2, "n_matches": 0}
    assert res["random_then_text"]["stored_members"] == 1 and res["255_values_once"]["stored_members"] == 1
    # one value: a literal, then a chain of length-258 matches at distance 1
    assert res["one_value"]["stored_members"] == 0 and res["one_value"]["out_bytes"] < 200 and res["one_value"]["n_matches"] == -(-(DC.PIECE - 1) // 258)
    assert res["run_lengths_3_to_258"]["n_matches"] >= 256 and res["distance_32768"]["n_matches"] > 0
    assert res["fastq_len_%d" % (2 * DC.PIECE + 1)]["n_members"] == 3
    assert res["fibonacci_counts_with_eob"]["stored_members"] == res["cl_deeper_than_7"]["stored_members"] == 0


@pytest.mark.gpu
def test_workgroups_that_build_a_second_member_leave_nothing_of_the_first():
    res = run_step("rounds", 240)
    print(res)
    assert res["n_members"] > 8 * 304 and res["distinct_pieces"] == 3 and res["stored_members"] == 1   # (the five bytes of the last piece)
    assert res["out_bytes"] < res["n_members"] * DC.PIECE * 6 // 10


@pytest.mark.gpu
def test_the_same_input_gives_the_same_bytes_on_every_run_and_handle():
    res = run_step("repeat", 120)
    print(res)
    assert res["level_2"] < res["level_1"] < res["level_0"]


@pytest.mark.gpu
def test_device_input_is_read_in_place_and_nothing_outside_it_counts():
    res = run_step("device_input", 120)
    print(res)
    assert len(res) == 5


@pytest.mark.gpu
def test_windows_of_every_size_stream_into_one_gzip_file_with_one_end_marker():
    res = run_step("streaming", 180)
    print(res)
    assert res["windows"] > 150


@pytest.mark.gpu
def test_a_text_deflated_from_the_device_parses_to_the_same_batch():
    res = run_step("handover", 120)
    print(res)
    assert res["records"] > 0 and res["packed"] < res["text"]


@pytest.mark.gpu
def test_the_programs_write_the_same_text_with_and_without_the_switch():
    res = run_step("programs", 600)
    print(res)
    assert sorted(res) == ["clean_adapter", "clean_lowqual", "correct_error_reads", "correct_error_reads_j1", "map_reads"]
    assert [len(res[p]) for p in ("clean_adapter", "clean_lowqual", "correct_error_reads", "correct_error_reads_j1")] == [1, 1, 1, 4]
    assert len(res["map_reads"]) >= 3
    assert all(members >= 1 for v in res.values() for _, _, members in v.values())


@pytest.mark.gpu
def test_the_error_returns():
    from dbg_assembly_amd import capi
    res = run_step("states", 120)
    print(res)
    want = {"level_3": capi.ERR_ARG, "level_above_the_built_ones": capi.ERR_ARG, "level_minus_1": capi.ERR_ARG,
            "results_before_a_call": capi.ERR_STATE, "device_before_a_call": capi.ERR_STATE, "n_bytes_2_to_the_31": capi.ERR_ARG,
            "n_bytes_2_to_the_31_device": capi.ERR_ARG, "misaligned_text": capi.ERR_ARG, "results_after_a_refused_call": capi.ERR_STATE,
            "empty_without_last": capi.OK, "empty_device_with_last": capi.OK, "own_output_as_input": capi.ERR_ARG,
            "results_after_refused_input": capi.OK, "capacity_one_short": capi.ERR_ARG, "capacity_exact": capi.OK, "null_info": capi.OK}
    assert res == want
