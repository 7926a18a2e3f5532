"""GPU: the INFLATE stage (csrc/dbgk_inflate.h) -- BGZF-framed gzip members to their bytes.  Every crafted member
(tests/inflate_cases.py: the project's own at three levels, zlib's at three levels and with fixed codes, stored blocks, hundreds of
blocks, flushes at every bit phase, hand-made blocks) against zlib byte for byte; corrupt members between good ones with zlib's
verdict and the expected reason each; more members than a round of the token area; repeated calls and a second handle; stream() at
windows that cut members everywhere; max_out_bytes; device input inside noise; Deflater -> Inflater -> Parser on the device; the
error returns; two programs with DBGK_GUNZIP=device.  Each GPU step is a child process under a time limit of its own
(tests/inflate_gpu_steps.py); the limits only end a stuck step.  The corrupt members belong on a device only behind the host sanitizer
run of the same decode core on the same members (tests/test_inflate_cpu.py, which runs without a GPU and is to be ordered first).  Every test here fails without the stage:
capi.Inflater does not exist."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_cases as IC  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "inflate_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_crafted_members_inflate_to_zlibs_bytes():
    res = run_step("crafted", 480)
    assert sorted(res) == ["own", "small", "zlib"]
    assert res["own"]["cases"] > 2000 and res["own"]["n_markers"] == res["own"]["cases"] and res["own"]["n_matches"] > 0
    assert res["zlib"]["n_stored"] > 0 and res["zlib"]["n_fixed"] > 0 and res["zlib"]["n_dynamic"] > 200
    # the end marker alone, four between members, and zlib's member of no bytes, which is the marker byte for byte
    assert res["small"]["n_markers"] == 6 and all(res[g]["n_bad"] == 0 for g in res)


@pytest.mark.gpu
def test_corrupt_members_get_zlibs_verdict_and_disturb_nothing():
    res = run_step("corrupt", 120)
    print(res)
    assert res["reasons"] == list(range(0, IC.R["FRAME"])) and res["members"] == 2 * res["bad"]


@pytest.mark.gpu
def test_more_members_than_a_round_of_the_token_area():
    res = run_step("rounds", 240)
    print(res)
    assert res["n_members"] > 20000 and res["n_bad"] == 0


@pytest.mark.gpu
def test_the_same_input_gives_the_same_bytes_verdicts_and_counters():
    res = run_step("repeat", 120)
    print(res)
    assert res["bad"] > 20 and res["members"] > res["bad"]


@pytest.mark.gpu
def test_windows_that_cut_members_everywhere_stream_to_the_same_text():
    from dbg_assembly_amd import capi
    res = run_step("streaming", 180)
    print(res)
    assert res.pop("tail_with_last") == capi.ERR_ARG
    assert sorted(res) == ["between_members", "inside_the_header", "inside_the_stream", "inside_the_trailer", "smaller_than_a_member", "the_whole_file"]
    assert res["the_whole_file"] == 1 and res["smaller_than_a_member"] > 100


@pytest.mark.gpu
def test_max_out_bytes_takes_whole_members_from_the_front():
    res = run_step("max_out", 120)
    assert res == {"1": 0, "65279": 0, "65280": 1, str(3 * 65280 + 1): 3}


@pytest.mark.gpu
def test_device_input_is_read_inside_the_tables_ranges_only():
    from dbg_assembly_amd import capi
    res = run_step("device_input", 180)
    print(res)
    assert res.pop("misaligned") == res.pop("offsets_decrease") == res.pop("offsets_past_the_buffer") == capi.ERR_ARG
    assert sorted(res) == ["front_16", "front_4128", "front_48"]


@pytest.mark.gpu
def test_deflated_text_inflates_and_parses_on_the_device_to_the_same_batch():
    res = run_step("roundtrip", 180)
    print(res)
    assert sorted(res) == ["level_0", "level_1", "level_2"] and res["level_2"]["packed"] < res["level_1"]["packed"] < res["level_0"]["packed"]


@pytest.mark.gpu
def test_the_error_returns():
    from dbg_assembly_amd import capi
    res = run_step("states", 120)
    print(res)
    want = {"max_out_2_to_the_31": capi.ERR_ARG, "results_before_a_call": capi.ERR_STATE, "device_before_a_call": capi.ERR_STATE,
            "status_before_a_call": capi.ERR_STATE, "n_bytes_2_to_the_31": capi.ERR_ARG, "plain_gzip": capi.ERR_ARG, "plain_text": capi.ERR_ARG,
            "other_subfield": capi.ERR_ARG, "isize_above_a_piece": capi.ERR_ARG, "cut_short_with_last": capi.ERR_ARG,
            "results_after_a_refused_call": capi.ERR_STATE, "n_bytes_2_to_the_31_device": capi.ERR_ARG, "misaligned_input": capi.ERR_ARG,
            "empty_without_last": capi.OK, "empty_with_last": capi.OK, "marker_alone": capi.OK, "own_output_as_input": capi.ERR_ARG,
            "results_after_refused_input": capi.OK, "capacity_one_short": capi.ERR_ARG, "capacity_exact": capi.OK, "status_capacity_short": capi.ERR_ARG,
            "null_info": capi.OK, "device_input_above_max_out": capi.ERR_ARG}
    assert res == want


@pytest.mark.gpu
def test_the_programs_read_bgzf_input_on_the_device_and_anything_else_through_zlib():
    res = run_step("programs", 600)
    print(res)
    assert sorted(res) == ["clean_lowqual_bgzf", "clean_lowqual_plain_gzip", "correct_error_reads_bgzf", "correct_error_reads_plain_gzip", "corrupt_message"]
    assert "member 0" in res["corrupt_message"]
