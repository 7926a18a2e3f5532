"""GPU: what the stage handles share (csrc/dbgk_host_stage.h) -- opening the device, closing, and the buffers that grow with a batch.
Every stage class of capi opened and closed; every create with a device index past the last, with -1, and with a parameter out of range;
one handle each of Formatter, Parser, Deflater and Inflater fed batches one below, at and one above the floor of each of its
capacities with a tiny batch in between, every output against the restatements byte for byte.  Each GPU step is a child process under a
time limit of its own (tests/stage_lifecycle_gpu_steps.py); the limits only end a stuck step."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = os.path.join(ROOT, "tests", "stage_lifecycle_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_every_stage_opens_and_closes_and_a_second_close_does_nothing():
    from dbg_assembly_amd import capi
    res = run_step("open_close", 120)
    print(res)
    classes = ("Corrector", "Mapper", "Pairer", "Parser", "Formatter", "Deflater", "Inflater", "Cleaner", "Scaffolder", "GapFiller", "SuperLinker",
               "ContigBuilder", "ContigBuilder_wide")
    assert all(res[c] == "closed" for c in classes) and res["together"] == len(classes)
    nulls = {k: v for k, v in res.items() if k.endswith("_destroy_null")}
    assert len(nulls) == 12 and set(nulls.values()) == {capi.ERR_ARG}


@pytest.mark.gpu
def test_a_device_index_past_the_last_is_a_hip_error_and_argument_checks_come_first():
    from dbg_assembly_amd import capi
    res = run_step("bad_device", 120)
    print(res)
    assert len(res) == 11
    for name, r in res.items():
        assert r["past_the_last"] == capi.ERR_HIP and r["error"] == "no usable HIP device", name
        assert r["minus_1"] == capi.ERR_ARG, name
        if name not in ("dbgk_clean_create", "dbgk_pair_create"):   # (the index is all these two take)
            assert r["bad_parameter"] == r["bad_parameter_past_the_last"] == capi.ERR_ARG, name


@pytest.mark.gpu
def test_buffers_regrown_at_their_floors_give_the_restatements_bytes():
    res = run_step("regrow", 240)
    print(res)
    f, p, z, i = res["format"], res["parse"], res["deflate"], res["inflate"]
    assert [f["records_%d" % n] for n in (16383, 16384, 16385)] == [4 * 16382, 4 * 16383, 4 * 16384]
    assert [f["text_%d" % n] for n in ((1 << 20) - 16, 1 << 20, (1 << 20) + 1)] == [(1 << 20) - 80, (1 << 20) - 64, (1 << 20) - 63]
    assert f["tiny_first"] == f["tiny_after_records"] == f["tiny_last"] == 15
    assert all("lines_%d" % n in p for n in (65535, 65536, 65537)) and [p["tiles_%d" % n] for n in (1023, 1024, 1025)] == [1023 << 12, 1 << 22, (1 << 22) + 1]
    assert p["tiny_first"] == p["tiny_after_lines"] == p["tiny_last"] == 14
    assert [z["slots_%d" % n] for n in (63, 64, 65, 66)] == [63, 64, 65, 66] and z["tiny_first"] == z["tiny_last"] == 2
    assert [i["members_%d" % n] for n in (1023, 1024, 1025)] == [1023, 1024, 1025] and (i["tiny_first"], i["tiny_last"]) == (2, 3)
