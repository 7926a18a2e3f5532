"""GPU: the life cycle of the graph handle (dbgk_handle), which owns its memory, events and streams through the owners of
csrc/dbgk_host_stage.h.  One handle of every shape of the struct opened and closed; creates that fail after the handle exists; the
buffers that grow with a device batch (start / dead bitmaps, prefix scratch, packed image, offsets) regrown small / large / small;
table resizes of the DIRECT and the PARTITION engine, the refused ones included.  Tables against the oracle or a second handle that
never took the path.  Each GPU step is a child process under a time limit of its own (tests/graph_lifecycle_gpu_steps.py); the
limits only end a stuck step."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = os.path.join(ROOT, "tests", "graph_lifecycle_gpu_steps.py")


def run_step(name, timeout=120):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_every_shape_of_the_graph_handle_opens_and_closes():
    from dbg_assembly_amd import capi
    res = run_step("open_close")
    print(res)
    shapes = ("direct", "direct_first_seen", "partition", "partition_one_shard", "kfreq_direct", "kfreq_hashed", "kfreq_blocks", "seedidx",
              "wide_atomic", "wide_records")
    assert all(res[s] == "closed" for s in shapes) and res["together"] == len(shapes)
    assert res["destroy_null"] == capi.ERR_ARG


@pytest.mark.gpu
def test_a_create_that_fails_leaves_no_handle_and_the_next_create_works():
    from dbg_assembly_amd import capi
    import graph_lifecycle_gpu_steps as S
    res = run_step("failed_create")
    print(res)
    assert set(res) == {"first_seen_on_partition", "device_past_the_last", "device_minus_1", "sharded_small_table"}
    assert all(r["status"] == capi.ERR_ARG for r in res.values())
    assert res["first_seen_on_partition"]["error"] == S.TRACK_MESSAGE
    assert len({r["nodes_after"] for r in res.values()}) == 1 and res["device_minus_1"]["nodes_after"] > 1000


@pytest.mark.gpu
def test_buffers_that_grow_with_a_device_batch_give_the_oracles_table():
    res = run_step("regrow")
    print(res)
    assert res["forms_of_the_large_batch"] and res["nodes"] > 1000


@pytest.mark.gpu
def test_resized_tables_hold_the_oracles_nodes_and_refused_resizes_leave_the_handle_usable():
    from dbg_assembly_amd import capi
    res = run_step("resize")
    print(res)
    assert res["direct_too_small"] == capi.ERR_TABLE_FULL
    assert res["partition_unfit"] == capi.ERR_ARG
    assert res["direct_nodes"] == res["partition_nodes"] == res["partition_nodes_after_refusal"] > 1000
