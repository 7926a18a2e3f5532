"""bench.py's plain run (set up, warm up, the timed steps, the line) and --dump-outputs: what the last timed step built, written
so that two builds of the project can be compared output for output."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--reads-per-gpu", "50000", "--genome-per-gpu", "400000", "--table-slots", "70000000", "--steps", "3", "--warmup", "1"]


def _bench(args, timeout=600):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)


def test_dump_outputs_needs_one_process():
    r = _bench(["--gpus", "2", "--dump-outputs", "unused"], timeout=120)
    assert r.returncode == 2 and "--dump-outputs needs one process" in r.stderr, r.stderr[-2000:]
    assert r.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_step_built(tmp_path, oracle):
    """The plain line and the --full --brief line of the same small cfg2 job: both time exactly --steps steps, only --full checks
    the graph, and both dump the same arrays -- the counters, digest and DepthStat of the table, and the node sample, which must
    be the one the CPU oracle's graph of the same reads gives."""
    import bench
    runs = []
    for name, extra in (("plain", []), ("full", ["--full", "--brief"])):
        d = tmp_path / name
        r = _bench(SMALL + ["--dump-outputs", str(d)] + extra)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout[:2000]
        out = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in out, key
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
        assert sorted(os.listdir(d)) == ["depth_stat.npy", "digest.npy", "nodes_sample.npy", "stats.npy"]
        arrays = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert all(a.dtype == np.float64 for a in arrays.values())
        runs.append((out, arrays))
    (plain, a), (full, b) = runs
    assert plain["verified"] is None
    assert full["verified"] and not full["verified"].startswith("not run"), full["verified"]
    for name in a:
        assert np.array_equal(a[name], b[name]), name

    P = oracle.synth_params(400000, 150, cfg=2)
    bases, offsets = oracle.synth_reads(P, 0, 50000)
    ref = oracle.build_graph(files_mem=[(bases, offsets)], k=31, init_hash_size=0.01, threads=4)
    assert a["stats"][:4].tolist() == [ref.total_reads, ref.total_kmers, ref.total_kmers, ref.count]
    assert plain["config"]["nodes"] == ref.count
    stub = types.SimpleNamespace(stats=types.SimpleNamespace(total_reads=0, total_kmers=0, stored_kmers=0, count=0, polyA_l_link=0,
                                                             polyA_r_link=0, other_bytes=0),
                                 digest=lambda: 0, link_stats=lambda cutoff: types.SimpleNamespace(depth_stat=[0] * 256),
                                 export_sorted=lambda: ref.nodes)
    want = bench.graph_outputs(stub, False, 50000 * 120)["nodes_sample"]
    assert len(want) > 1000 and np.array_equal(a["nodes_sample"], want)
