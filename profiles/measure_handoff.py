"""From raw reads to a finalized k = 31 graph of the CORRECTED reads, two routes on the same binary (10 M x 150 bp, corrector
k = 17, table from a KFREQ handle at cutoff 2, batches of 1 M reads):

  (a) today's route   per batch dbgk_corr_reads (upload, kernels, download of every untrimmed byte), the host trim, dbgk_push_reads
  (b) the new route   per batch ONE upload, dbgk_push_reads_device into KFREQ; dbgk_corr_from_kfreq; per batch
                      dbgk_corr_reads_device, dbgk_corr_compact, dbgk_push_corrected

Each route runs --reps times.  Reported per run: the wall time of the whole route and of its stages (creating the handles is a
stage of its own, the same work in both routes, and is left out of the comparison), and the wall time WITHOUT
the corrector's own kernels (classify + correct + overflow device ms, which both routes run alike).  The project's rule decides
whether the routes separate: the slowest run of the new route against the fastest of the old.  Next to it the gather's rate
(kept bytes read + bytes written per second of k_emit_gather_lds) and dbgk_measure_copy_bandwidth of the same run.  Writes
profiles/handoff_measure.json; without a GPU it lists the figures that are missing.  Reported, not gated.

    python profiles/measure_handoff.py [--reads 10000000] [--genome 5000000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "handoff_measure.json")
FIGURES = ["route_a wall_s (3 runs)", "route_b wall_s (3 runs)", "wall_s without the corrector's kernels, both routes", "routes_separate",
           "gather GB/s (bytes read + written)", "copy_bandwidth GB/s of the same run", "ms_scan", "ms_gather"]
K_CORR, K_GRAPH, CUTOFF, READ_LEN = 17, 31, 2, 150


def host_trim(out, offsets, rec):
    """the host loop of bin/correct_error_reads (host/correct_error_reads.cpp:151-174) without its text: the kept bytes of every
    read back to back and their offsets, deleted reads empty.  A numpy stand-in for the C++ loop (one boolean mask over the batch,
    all reads READ_LEN long); its time is reported as a stage of its own, and the routes are also compared without it"""
    n = len(rec)
    lt, rt = rec["left_trim"].astype(np.int32), rec["right_trim"].astype(np.int32)
    lens = np.where(rec["deleted"] != 0, 0, READ_LEN - lt - rt)
    col = np.arange(READ_LEN, dtype=np.int32)[None, :]
    keep = (col >= lt[:, None]) & (col < (lt + lens)[:, None])
    coff = np.zeros(n + 1, dtype=np.uint64)
    coff[1:] = np.cumsum(lens)
    return out.reshape(n, READ_LEN)[keep], coff


def graph(capi, n_reads):
    return capi.Graph(k=K_GRAPH, table_slots=capi.find_next_prime_ref(max(n_reads * 100, 1 << 27)), engine=capi.ENGINE_PARTITION,
                      max_read_len=250, expected_kmers=n_reads * (READ_LEN - K_GRAPH + 1))


def kfreq(capi, batch):
    return capi.Graph(k=K_CORR, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000, expected_kmers=batch * (READ_LEN - K_CORR + 1))


def kernel_ms(st):
    return st["ms_classify"] + st["ms_correct"] + st["ms_overflow"]


def route_a(capi, batches):
    t = {"create": 0.0, "kfreq": 0.0, "table": 0.0, "correct": 0.0, "trim": 0.0, "push": 0.0, "finalize": 0.0}
    ms = 0.0
    n = sum(len(o) - 1 for _, o in batches)
    t0 = time.perf_counter()
    with kfreq(capi, len(batches[0][1]) - 1) as kf, capi.Corrector(k=K_CORR) as c, graph(capi, n) as g:
        t["create"] = time.perf_counter() - t0   # the three handles: 16 GiB of counters, the 1-bit table, the graph's table and store
        t1 = time.perf_counter()
        for bases, offsets in batches:
            kf.push_reads(bases, offsets)
        kf.finalize()
        t["kfreq"] = time.perf_counter() - t1
        t1 = time.perf_counter()
        c.from_kfreq(kf, CUTOFF)
        t["table"] = time.perf_counter() - t1
        for bases, offsets in batches:
            t1 = time.perf_counter()
            out, rec = c.correct(bases, offsets)
            t2 = time.perf_counter()
            tb, to = host_trim(out, offsets, rec)
            t3 = time.perf_counter()
            g.push_reads(tb, to)
            t4 = time.perf_counter()
            t["correct"] += t2 - t1
            t["trim"] += t3 - t2
            t["push"] += t4 - t3
            ms += kernel_ms(c.batch_stats())
        t1 = time.perf_counter()
        st = g.finalize()
        t["finalize"] = time.perf_counter() - t1
        wall = time.perf_counter() - t0
        nodes = int(st.count)
    return {"wall_s": wall, "corrector_kernel_ms": ms, "wall_s_without_corrector_kernels": wall - ms / 1e3, "stages_s": t, "nodes": nodes}


def route_b(capi, batches):
    t = {"create": 0.0, "upload": 0.0, "kfreq": 0.0, "table": 0.0, "correct": 0.0, "compact": 0.0, "push": 0.0, "finalize": 0.0}
    ms = ms_scan = ms_gather = 0.0
    moved = 0
    n = sum(len(o) - 1 for _, o in batches)
    t0 = time.perf_counter()
    with kfreq(capi, len(batches[0][1]) - 1) as kf, capi.Corrector(k=K_CORR) as c, graph(capi, n) as g:
        t["create"] = time.perf_counter() - t0
        bufs = []
        for bases, offsets in batches:
            t1 = time.perf_counter()
            d_b, d_o = kf.malloc(bases.size + 64), kf.malloc(offsets.nbytes)
            d_b.from_host(bases)
            d_o.from_host(offsets)
            t2 = time.perf_counter()
            kf.push_reads_device(d_b.ptr, d_o.ptr, len(offsets) - 1, bases.size)
            t["upload"] += t2 - t1
            t["kfreq"] += time.perf_counter() - t2
            bufs.append((d_b, d_o))
        t1 = time.perf_counter()
        kf.finalize()
        t["kfreq"] += time.perf_counter() - t1
        t1 = time.perf_counter()
        c.from_kfreq(kf, CUTOFF)
        t["table"] = time.perf_counter() - t1
        for (bases, offsets), (d_b, _) in zip(batches, bufs):
            t1 = time.perf_counter()
            c.correct_device(d_b.ptr, offsets)
            t2 = time.perf_counter()
            info = c.compact()
            t3 = time.perf_counter()
            g.push_corrected(c)
            t4 = time.perf_counter()
            t["correct"] += t2 - t1
            t["compact"] += t3 - t2
            t["push"] += t4 - t3
            ms += kernel_ms(c.batch_stats())
            ms_scan += info["ms_scan"]
            ms_gather += info["ms_gather"]
            moved += info["result_bases"] + (info["result_bases"] + 15) // 16 * 16
        t1 = time.perf_counter()
        st = g.finalize()
        t["finalize"] = time.perf_counter() - t1
        wall = time.perf_counter() - t0
        nodes = int(st.count)
        for d_b, d_o in bufs:
            d_b.free()
            d_o.free()
    return {"wall_s": wall, "corrector_kernel_ms": ms, "wall_s_without_corrector_kernels": wall - ms / 1e3, "stages_s": t, "nodes": nodes,
            "ms_scan": ms_scan, "ms_gather": ms_gather, "gather_bytes": moved, "gather_gbps": moved / (ms_gather * 1e6) if ms_gather else None}


def rounded(x):
    if isinstance(x, float):
        return round(x, 4)
    if isinstance(x, dict):
        return {k: rounded(v) for k, v in x.items()}
    if isinstance(x, list):
        return [rounded(v) for v in x]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--batch", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    job = dict(reads=a.reads, read_len=READ_LEN, genome=a.genome, batch=a.batch, k_corrector=K_CORR, k_graph=K_GRAPH, cutoff=CUTOFF, reps=a.reps)
    if capi.lib().dbgk_device_count() < 1:
        with open(OUT, "w") as f:
            json.dump({"job": job, "missing": FIGURES, "note": "no GPU on the machine this file was written on: nothing here is measured"}, f, indent=1)
            f.write("\n")
        print("no GPU: wrote the list of missing figures to", OUT)
        return
    from oracle import oracle_py as O
    P = O.synth_params(a.genome, READ_LEN, sub_rate=0.01, n_rate=0.002, cfg=11)
    batches = [O.synth_reads(P, first, min(a.batch, a.reads - first)) for first in range(0, a.reads, a.batch)]
    runs_a, runs_b = [], []
    for _ in range(a.reps):   # interleaved, so that a drift of the machine meets both routes
        runs_a.append(route_a(capi, batches))
        runs_b.append(route_b(capi, batches))
    assert len({r["nodes"] for r in runs_a + runs_b}) == 1, "the two routes built different graphs"
    with capi.Graph(k=K_GRAPH, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:   # (any handle: the call needs a stream)
        copy_gbps = g.copy_bandwidth(2 << 30, 5)
    key = "wall_s_without_corrector_kernels"
    for r in runs_a + runs_b:   # the route proper: creating the three handles is the same work in both routes
        r["route_s"] = r[key] - r["stages_s"]["create"]
    fast_a, slow_b = min(r["route_s"] for r in runs_a), max(r["route_s"] for r in runs_b)
    fast_a_no_trim = min(r["route_s"] - r["stages_s"]["trim"] for r in runs_a)   # as if the host trim cost nothing
    fast_a_wall, slow_b_wall = min(r[key] for r in runs_a), max(r[key] for r in runs_b)
    gather = [r["gather_gbps"] for r in runs_b if r["gather_gbps"] is not None]   # (None: a run in which nothing was kept)
    out = {"job": job, "route_a_today": runs_a, "route_b_device": runs_b,
           "rule": ("the slowest run of the new route against the fastest run of the old; compared is route_s = wall time without the "
                    "corrector's kernels and without the creation of the three handles (stage `create`: identical work in both routes, "
                    "16 GiB of counters and the graph's table, and it varied between runs by more than the routes differ)"),
           "with_handle_creation": {"fastest_a_s": fast_a_wall, "slowest_b_s": slow_b_wall, "routes_separate": bool(slow_b_wall < fast_a_wall)},
           "fastest_a_s": fast_a, "slowest_b_s": slow_b, "routes_separate": bool(slow_b < fast_a),
           "speedup_slowest_b_vs_fastest_a": fast_a / slow_b,
           "fastest_a_without_host_trim_s": fast_a_no_trim, "routes_separate_without_host_trim": bool(slow_b < fast_a_no_trim),
           "routes_separate_caveat": ("route (a)'s trim stage is a numpy stand-in for the C++ loop of bin/correct_error_reads, not that "
                                      "code: routes_separate depends on a stage that is not the real host code.  "
                                      "routes_separate_without_host_trim charges route (a) nothing for the trim and is the verdict "
                                      "that does not depend on the stand-in"),
           "gather_gbps": gather, "copy_bandwidth_gbps": copy_gbps, "gather_over_copy": [v / copy_gbps for v in gather],
           "gather_time": "ms_gather is the device time of k_emit_gather_lds alone (events directly around the kernel)"}
    if gather and max(gather) < 0.5 * copy_gbps:
        out["gather_bound"] = {
            "observed": "the gather stays below half the copy rate of this run (gather_over_copy)",
            "hypothesis_not_profiled": ("not HBM.  By its instruction count the kernel is bound by LDS byte stores and per-tile latency: a "
                                        "4 KiB tile takes 1024 aligned 4-byte source loads and 4096 ds_write_b8 (64 wave-instructions of LDS "
                                        "byte stores against 4 for the 16-byte read-out), behind two dependent 64-way searches of 3-4 "
                                        "loads each and three barriers per pass over 256 reads.  No counter run has confirmed this")}
    with open(OUT, "w") as f:
        json.dump(rounded(out), f, indent=1)
        f.write("\n")
    print(json.dumps(rounded({k: out[k] for k in ("fastest_a_s", "slowest_b_s", "routes_separate", "routes_separate_without_host_trim",
                                                  "gather_gbps", "copy_bandwidth_gbps")})))


if __name__ == "__main__":
    main()
