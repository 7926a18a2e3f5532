"""GPU (-m gpu): the product multi-GPU path (HipEngine + torch.distributed/NCCL=RCCL collectives)
on the one GPU a test box has: a single-rank process group exercises the same code the 8-GPU
bench runs (count all-reduce, all-to-all of nodes through torch CUDA tensors, owner merge into a
reset table, scalar all-reduce).  world > 1 plumbing is covered on CPU by test_multigpu_gloo.py."""
import os
import socket

import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("engine", [1, 2])
def test_exchange_and_merge_single_rank_nccl(engine):
    import torch
    import torch.distributed as dist
    from dbg_assembly_amd import capi
    from dbg_assembly_amd.multigpu import HipEngine, exchange_and_merge

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        n_reads, G = 300000, 2000000
        P = capi.synth_params(G, 150, cfg=2)
        size = capi.find_next_prime_ref(80000000)
        with capi.Graph(k=31, table_slots=size, engine=engine, expected_kmers=n_reads * 150) as g:
            d_bases, d_off, nb = g.synth_reads_device(P, 0, n_reads)
            g.push_reads_device(d_bases.ptr, d_off.ptr, n_reads, nb)
            st = g.finalize()
            want = (st.count, st.total_kmers, st.total_reads, g.digest())
            out = exchange_and_merge(HipEngine(g, torch.device("cuda", 0)))
            assert (out["count"], out["total_kmers"], out["total_reads"]) == want[:3]
            assert out["sent_nodes"] == out["recv_nodes"] == st.count
            assert g.digest() == want[3]          # the owner table after the exchange == the local table
            # and the handle is reusable for the next step (bench loop)
            g.reset()
            g.push_reads_device(d_bases.ptr, d_off.ptr, n_reads, nb)
            st2 = g.finalize()
            assert (st2.count, g.digest()) == (want[0], want[3])
            d_bases.free()
            d_off.free()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("expected", [0, 200000 * 150])
def test_exchange_and_merge_wide_single_rank_nccl(expected):
    """`bench.py --config cfg5` on several GPUs: the same flow with 32-byte nodes (WideHipEngine), the local graph built
    by the fused-atomic kernels (expected = 0) or through records"""
    import torch
    import torch.distributed as dist
    from dbg_assembly_amd import capi
    from dbg_assembly_amd.multigpu import WideHipEngine, exchange_and_merge

    torch.cuda.set_device(0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        n_reads, G = 200000, 1500000
        P = capi.synth_params(G, 150, sub_rate=0.001, cfg=5)
        size = capi.find_next_prime_ref(1 << 26)
        with capi.Graph(k=63, table_slots=size, engine=capi.ENGINE_WIDE, expected_kmers=expected) as g:
            d_bases, d_off, nb = g.synth_reads_device(P, 0, n_reads)
            for _ in range(2):   # two steps: the handle must be reusable (bench loop)
                g.reset()
                g.push_reads_device(d_bases.ptr, d_off.ptr, n_reads, nb)
                st = g.finalize()
                want = (st.count, st.total_kmers, st.total_reads, g.digest())
                out = exchange_and_merge(WideHipEngine(g, torch.device("cuda", 0)))
                assert (out["count"], out["total_kmers"], out["total_reads"]) == want[:3]
                assert out["sent_nodes"] == out["recv_nodes"] == st.count
                assert g.digest() == want[3]
            d_bases.free()
            d_off.free()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("chunks", [8, 1])
def test_sharded_finalize_single_rank_nccl(oracle, chunks):
    """slot-range ownership flow of bench.py (N > 1) with a one-rank shard: the all-to-all runs on
    the library's own device buffers wrapped as torch tensors, the handed-over nodes wrap around to
    the same shard; result == plain single-GPU build == oracle"""
    import numpy as np
    import torch
    import torch.distributed as dist
    from dbg_assembly_amd import capi
    from dbg_assembly_amd.multigpu import sharded_finalize

    torch.cuda.set_device(0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        n_reads, G = 100000, 500000
        P, PO = capi.synth_params(G, 150, cfg=2), oracle.synth_params(G, 150, cfg=2)
        bases, offsets = oracle.synth_reads(PO, 0, n_reads)
        size = capi.find_next_prime_ref(70000000)
        with capi.Graph(k=31, table_slots=size, engine=capi.ENGINE_PARTITION, expected_kmers=n_reads * 150,
                        shard_count=1, shard_index=0) as g:
            d_bases, d_off, nb = g.synth_reads_device(P, 0, n_reads)
            for _ in range(2):  # two steps: the handle must be reusable (bench loop)
                g.reset()
                g.push_reads_device(d_bases.ptr, d_off.ptr, n_reads, nb)
                out = sharded_finalize(g, torch.device("cuda", 0), exchange_chunks=chunks)
            nodes = g.export_sorted()
            d_bases.free()
            d_off.free()
        ref = oracle.build_graph(files_mem=[(bases, offsets)], k=31, init_hash_size=0.02)
        assert (out["count"], out["total_kmers"], out["total_reads"]) == (ref.count, ref.total_kmers, ref.total_reads)
        assert out["records_global"] == ref.total_kmers  # no key-0 k-mers in this input
        assert np.array_equal(nodes, ref.nodes)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("extra", [[], ["--exchange", "nodes"], ["--exchange-chunks", "1"]])
def test_bench_multi_gpu_code_path_rehearsal(extra):
    """bench.py's N > 1 branch (process group, shard, exchange, JSON assembly) with the one rank a test box
    has; stdout must carry exactly one line, the JSON record (RCCL prints a banner when a communicator is
    created)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--force-sharded", "--reads-per-gpu", "300000",
                        "--genome-per-gpu", "2000000", "--table-slots", "80000000", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--full"] + extra, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:2000]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["config"]["nodes"] > 1000000 and out["value"] > 0
    for key in ("metric", "unit", "ms_per_step", "roofline", "scaling", "dtype", "data"):
        assert key in out


@pytest.mark.parametrize("n_passes", [1, 2])
def test_wide_sharded_build_single_rank_nccl(n_passes):
    """`bench.py --config cfg5 --gpus N`: the slot-range flow for 128-bit keys (multigpu.wide_sharded_build: passes over the
    input, bucket-count all-reduce, all-to-all of the 16-byte record buckets in pieces with the exchange verified, region
    builds, hand-offs, side-table gather) on one rank over RCCL, against a plain WIDE handle of the same reads; twice on
    one handle (bench loop)"""
    import torch
    import torch.distributed as dist
    from dbg_assembly_amd import capi
    from dbg_assembly_amd.multigpu import wide_sharded_build

    torch.cuda.set_device(0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        n_reads, G, k = 200000, 1500000, 63
        P = capi.synth_params(G, 150, sub_rate=0.001, cfg=5)
        size = capi.find_next_prime_ref(1 << 26)
        device = torch.device("cuda", 0)
        with capi.Graph(k=k, table_slots=size, engine=capi.ENGINE_WIDE, expected_kmers=n_reads * 88) as ref:
            d_bases, d_off, nb = ref.synth_reads_device(P, 0, n_reads)
            ref.push_reads_device(d_bases.ptr, d_off.ptr, n_reads, nb)
            st = ref.finalize()
            want = (int(st.count), int(st.total_kmers), int(st.total_reads), ref.digest())
            with capi.Graph(k=k, table_slots=size, engine=capi.ENGINE_WIDE, expected_kmers=n_reads * 88, shard_count=1, shard_index=0,
                            n_passes=n_passes) as g:
                assert g.wide_pass_info()[0] == n_passes
                for _ in range(2):
                    g.reset()
                    out = wide_sharded_build(g, device, lambda h: h.push_reads_device(d_bases.ptr, d_off.ptr, n_reads, nb), exchange_chunks=4,
                                             verify_exchange=True)
                    assert (out["count"], out["total_kmers"], out["total_reads"], g.digest()) == want
                    assert out["passes"] == n_passes and out["records_global"] <= want[1]
            d_bases.free()
            d_off.free()
    finally:
        dist.destroy_process_group()


SMALL = ["--reads-per-gpu", "200000", "--genome-per-gpu", "1500000", "--table-slots", "40000000", "--steps", "2", "--warmup", "1",
         "--no-cpu-baseline", "--full"]


@pytest.mark.parametrize("extra", [
    ["--gpus", "2"],                                                   # cfg2's flow: slot-range shards, records exchanged in pieces
    ["--gpus", "3", "--exchange-chunks", "3"],                         # 29 level-1 buckets over 3 ranks: the last rank owns fewer
    ["--gpus", "2", "--exchange", "nodes", "--table-slots", "80000000"],   # hash ownership, aggregated nodes exchanged (local tables)
    ["--gpus", "2", "--config", "cfg5"],                               # k = 63: 16-byte records, 32-byte nodes, side tables gathered
    ["--gpus", "3", "--config", "cfg5", "--passes", "2"],              # ... in two passes over the input
    ["--gpus", "2", "--config", "cfg4", "--kmer", "14"],               # frequency tables, saturating reduce-scatter
], ids=lambda e: "_".join(x.lstrip("-") for x in e))
def test_several_ranks_on_one_gpu_build_the_whole_jobs_graph(extra):
    """The N > 1 flows with N REAL ranks -- real handles, real kernels, every rank its own reads and its own shard -- on the one
    GPU a test box has: `bench.py --gpus N --backend gloo --one-gpu` (RCCL refuses two ranks on one device, so the collectives
    are staged through host memory: multigpu.py 'transport'; everything else is the code the 8-GPU run executes).  After its
    timed loop bench.py adds up count / k-mer total / node digest / DepthStat over the ranks and compares them with the WHOLE
    job rebuilt on rank 0 by the atomic engine (cfg4: checksums of the owned counter ranges against the whole-job table); a
    mismatch is a non-zero exit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--backend", "gloo", "--one-gpu"] + SMALL + extra,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[:2000]
    out = json.loads(lines[0])
    assert out["n_gpus"] == int(extra[1])
    assert out["verified"] and "== the" in out["verified"] and not out["verified"].startswith("not run"), out["verified"]
    if "cfg4" not in extra:
        assert out["config"]["nodes"] > 1000000


@pytest.mark.parametrize("world,rank", [(2, 1), (4, 0), (8, 7)])
def test_plan_partition_equals_the_geometry_a_sharded_handle_really_gets(world, rank):
    """dbgk_plan_partition (the device-free planner behind `bench.py --plan-only`) must say what a real sharded handle of the same
    parameters reports through dbgk_shard_buffers: slot range, buckets per rank and own buckets, bucket and chunk sizes -- for cfg2's
    per-GPU share at N = 2, 4, 8 (small record stores: only the geometry matters here)"""
    from dbg_assembly_amd import capi
    per_gpu = min(600_000_000, (2 ** 32 - 2 ** 22) // world)
    size = capi.find_next_prime_ref(per_gpu * world)
    expected = 4_000_000
    plan = capi.plan_partition(size, expected, world, rank)
    with capi.Graph(k=31, table_slots=size, engine=capi.ENGINE_PARTITION, expected_kmers=expected, shard_count=world, shard_index=rank) as g:
        info = g.shard_info()
        assert (int(info.n_ranks), int(info.rank), int(info.table_slots_global)) == (world, rank, size)
        assert (int(info.slot_lo), int(info.slot_hi)) == (int(plan.slot_lo), int(plan.slot_hi))
        assert (int(info.buckets_per_rank), int(info.own_buckets)) == (int(plan.buckets_per_rank), int(plan.own_buckets))
        assert int(info.bucket_bytes) == int(plan.records_per_level1_bucket) * 8
        assert int(info.chunk_bytes) == int(plan.buckets_per_rank) * int(plan.records_per_level1_bucket) * 8
        assert int(plan.inbox_bytes) == world * int(info.chunk_bytes) == int(plan.level1_store_bytes)
        assert int(plan.table_bytes) == (int(info.slot_hi) - int(info.slot_lo)) * 16
