"""The PAIR stage on 2 x 10 M x 150 bp with about 10 % of the reads of either mate file emptied (in batches of 1 M pairs), and raw
mates -> hits on two routes of the same binary.  Both routes start from the two compact batches as two correctors hold them
(dbgk_corr_compact_from with records that delete every tenth read: the same work in both routes, reported as a stage of its own and
left out of the comparison):

  (a) today's route   both compact_to_host calls, the host merge into the pair batch (a numpy stand-in for the loop of
                      merge_two_corr_files), Mapper.map (upload of the pair batch)
  (b) the new route   Pairer.split_device on the two compact_device results, Mapper.map_device on the PAIRED output where it lies

Each route runs --reps times, interleaved.  Reported:
  1. ms_rank (classify + flag scans + scatter + offset scans) and ms_gather (both outputs) summed over the batches of a run;
  2. the gather's rate (bytes read + 16-byte vectors written, both outputs, one plane) next to dbgk_measure_copy_bandwidth of the same
     run and next to the emit gather of the corrector (k_emit_gather_lds, one plane) on an output of the same size: the PAIRED
     output of the first batch, compacted untrimmed;
  3. the wall time of each route and of its stages.  The project's rule decides whether the routes separate: the slowest run of
     the new route against the fastest of the old.  The host merge of route (a) is a numpy stand-in, so the verdict is also given
     with the merge charged nothing.
Writes profiles/pair_measure.json; without a GPU it lists the figures that are missing.  Reported, not gated.

    python profiles/measure_pair.py [--pairs 10000000] [--genome 5000000] [--batch 1000000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "pair_measure.json")
FIGURES = ["ms_rank and ms_gather of the pair split (3 runs)", "pair gather GB/s (bytes read + written, both outputs, one plane)",
           "copy_bandwidth GB/s of the same run", "k_emit_gather_lds GB/s on an output of the same size",
           "route_a wall_s (3 runs)", "route_b wall_s (3 runs)", "routes_separate"]
READ_LEN, K, S, MIN_READ, IDENTITY = 150, 31, 5, 30, 0.97


def make_batch(capi, O, P, first, n, seed):
    """n pairs: mate 1 = generator reads [first, first + n), mate 2 = the n reads behind them; every tenth read of either is deleted"""
    rng = np.random.default_rng(seed)
    mates = []
    for m in range(2):
        bases, offsets = O.synth_reads(P, 2 * first + m * n, n)
        rec = np.zeros(n, dtype=capi.CORR_REC_DTYPE)
        rec["deleted"] = rng.random(n) < 0.1
        mates.append((np.ascontiguousarray(bases, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.uint64), rec))
    return mates


def host_merge(b1, o1, b2, o2):
    """the PAIRED batch of merge_two_corr_files on the host, all kept reads READ_LEN long: a numpy stand-in for its loop"""
    l1, l2 = np.diff(o1.astype(np.int64)), np.diff(o2.astype(np.int64))
    i = np.flatnonzero((l1 > 0) & (l2 > 0))
    out = np.empty((len(i), 2, READ_LEN), dtype=np.uint8)
    col = np.arange(READ_LEN, dtype=np.int64)[None, :]
    out[:, 0, :] = b1[o1[:-1].astype(np.int64)[i][:, None] + col]
    out[:, 1, :] = b2[o2[:-1].astype(np.int64)[i][:, None] + col]
    off = np.arange(2 * len(i) + 1, dtype=np.uint64) * np.uint64(READ_LEN)
    return out.reshape(-1), off


def compact_both(correctors, mates):
    for c, (bases, offsets, rec) in zip(correctors, mates):
        c.compact_from(bases, offsets, rec)


def route_a(capi, correctors, mapper, batches):
    t = {"compact": 0.0, "to_host": 0.0, "host_merge": 0.0, "map": 0.0}
    mapped = reads = 0
    t0 = time.perf_counter()
    for mates in batches:
        t1 = time.perf_counter()
        compact_both(correctors, mates)
        t2 = time.perf_counter()
        (b1, o1), (b2, o2) = correctors[0].compact_to_host(), correctors[1].compact_to_host()
        t3 = time.perf_counter()
        bases, off = host_merge(b1, o1, b2, o2)
        t4 = time.perf_counter()
        hits = mapper.map(bases, off)
        t5 = time.perf_counter()
        for name, dt in (("compact", t2 - t1), ("to_host", t3 - t2), ("host_merge", t4 - t3), ("map", t5 - t4)):
            t[name] += dt
        mapped += int((hits["contig"][:, 0] != -1).sum())
        reads += len(hits)
    wall = time.perf_counter() - t0
    return {"wall_s": wall, "route_s": wall - t["compact"], "stages_s": t, "pair_reads": reads, "mapped": mapped}


def route_b(capi, correctors, pairer, mapper, batches):
    t = {"compact": 0.0, "split": 0.0, "map": 0.0}
    ms = [0.0, 0.0]
    moved = mapped = reads = 0
    t0 = time.perf_counter()
    for mates in batches:
        n = len(mates[0][1]) - 1
        t1 = time.perf_counter()
        compact_both(correctors, mates)
        t2 = time.perf_counter()
        (d_b1, d_o1, _, _), (d_b2, d_o2, _, _) = correctors[0].compact_device(), correctors[1].compact_device()
        info = pairer.split_device(d_b1, d_o1, d_b2, d_o2, n)
        t3 = time.perf_counter()
        d_b, _, d_o, n_out, nb = pairer.device(capi.PAIR_PAIRED)
        hits = mapper.map_device(d_b, d_o, n_out, nb, info["max_len"])
        t4 = time.perf_counter()
        for name, dt in (("compact", t2 - t1), ("split", t3 - t2), ("map", t4 - t3)):
            t[name] += dt
        ms[0] += info["ms_rank"]
        ms[1] += info["ms_gather"]
        moved += sum(x + (x + 15) // 16 * 16 for x in (info["pair_bases"], info["single_bases"]))
        mapped += int((hits["contig"][:, 0] != -1).sum())
        reads += len(hits)
    wall = time.perf_counter() - t0
    return {"wall_s": wall, "route_s": wall - t["compact"], "stages_s": t, "pair_reads": reads, "mapped": mapped, "ms_rank": ms[0],
            "ms_gather": ms[1], "gather_bytes": moved, "gather_gbps": moved / (ms[1] * 1e6) if ms[1] else None}


def emit_gather_same_size(capi, correctors, pairer, mates):
    """k_emit_gather_lds on the PAIRED output of the first batch, compacted untrimmed: one plane of the same output size
    -> (GB/s of bytes read + written, ms, output bytes)"""
    n = len(mates[0][1]) - 1
    compact_both(correctors, mates)
    (d_b1, d_o1, _, _), (d_b2, d_o2, _, _) = correctors[0].compact_device(), correctors[1].compact_device()
    pairer.split_device(d_b1, d_o1, d_b2, d_o2, n)
    bases, _, off, _ = pairer.results(capi.PAIR_PAIRED)
    rec = np.zeros(len(off) - 1, dtype=capi.CORR_REC_DTYPE)
    best = None
    for _ in range(3):
        info = correctors[0].compact_from(bases, off, rec)
        assert info["result_bases"] == bases.size
        best = info["ms_gather"] if best is None else min(best, info["ms_gather"])
    total = int(bases.size)
    return (total + (total + 15) // 16 * 16) / (best * 1e6), best, total


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
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--batch", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    job = dict(pairs=a.pairs, read_len=READ_LEN, emptied=0.1, genome=a.genome, batch=a.batch, k=K, s=S, min_read_len=MIN_READ, min_identity=IDENTITY,
               reps=a.reps)
    if capi.lib().dbgk_device_count() < 1:
        with open(a.out, "w") as f:
            json.dump({"job": job, "missing": FIGURES, "note": "no GPU on the machine this file was written on: nothing here is measured"}, f, indent=1)
            f.write("\n")
        print("no GPU: wrote the list of missing figures to", a.out)
        return
    from oracle import oracle_py as O
    cb, co = O.synth_reads(O.synth_params(a.genome, 5000, sub_rate=0.0, n_rate=0.0, cfg=7), 0, a.genome // 5000)
    contigs = [cb[int(co[i]):int(co[i + 1])].tobytes() for i in range(len(co) - 1)]
    P = O.synth_params(a.genome, READ_LEN, sub_rate=0.01, n_rate=0.001, cfg=7)
    batches = [make_batch(capi, O, P, first, min(a.batch, a.pairs - first), first) for first in range(0, a.pairs, a.batch)]
    correctors = [capi.Corrector(k=9), capi.Corrector(k=9)]   # (compact_from needs no table)
    runs_a, runs_b = [], []
    with capi.Pairer() as pairer, capi.Mapper(k=K, s=S, r=MIN_READ, identity=IDENTITY, second_alignment=False) as mapper:
        mapper.set_contigs(contigs)
        for _ in range(a.reps):   # interleaved, so that a drift of the machine meets both routes
            runs_a.append(route_a(capi, correctors, mapper, batches))
            runs_b.append(route_b(capi, correctors, pairer, mapper, batches))
        emit_gbps, emit_ms, emit_bytes = emit_gather_same_size(capi, correctors, pairer, batches[0])
    for c in correctors:
        c.close()
    assert len({(r["pair_reads"], r["mapped"]) for r in runs_a + runs_b}) == 1, "the two routes mapped different reads"
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:   # (any handle: the call needs a stream)
        copy_gbps = g.copy_bandwidth(2 << 30, 5)
    fast_a, slow_b = min(r["route_s"] for r in runs_a), max(r["route_s"] for r in runs_b)
    fast_a_no_merge = min(r["route_s"] - r["stages_s"]["host_merge"] for r in runs_a)
    out = {"job": job, "route_a_today": runs_a, "route_b_device": runs_b,
           "rule": ("the slowest run of the new route against the fastest run of the old; compared is route_s = wall time without the stage "
                    "`compact` (dbgk_corr_compact_from of both mate batches: identical work in both routes)"),
           "fastest_a_s": fast_a, "slowest_b_s": slow_b, "routes_separate": bool(slow_b < fast_a), "speedup_slowest_b_vs_fastest_a": fast_a / slow_b,
           "fastest_a_without_host_merge_s": fast_a_no_merge, "routes_separate_without_host_merge": bool(slow_b < fast_a_no_merge),
           "routes_separate_caveat": ("route (a)'s host_merge is a numpy stand-in for the loop of merge_two_corr_files, not that code; "
                                      "routes_separate_without_host_merge charges route (a) nothing for it and is the verdict that does not "
                                      "depend on the stand-in"),
           "ms_rank": [r["ms_rank"] for r in runs_b], "ms_gather": [r["ms_gather"] for r in runs_b],
           "gather_gbps": [r["gather_gbps"] for r in runs_b], "copy_bandwidth_gbps": copy_gbps,
           "gather_over_copy": [r["gather_gbps"] / copy_gbps if r["gather_gbps"] else None for r in runs_b],
           "gather_bytes_counted": "per output the bytes read and the 16-byte vectors written; one plane (no qualities), both outputs",
           "emit_gather_same_output_size": {"gbps": emit_gbps, "ms_gather_best_of_3": emit_ms, "output_bytes": emit_bytes,
                                            "note": "k_emit_gather_lds, one plane, the PAIRED output of the first batch compacted untrimmed"},
           "gather_time": "ms_gather is the device time from in front of the first to behind the second k_pair_gather launch of a split"}
    with open(a.out, "w") as f:
        json.dump(rounded(out), f, indent=1)
        f.write("\n")
    print(json.dumps(rounded({k: out[k] for k in ("fastest_a_s", "slowest_b_s", "routes_separate", "routes_separate_without_host_merge", "ms_rank",
                                                  "ms_gather", "gather_gbps", "copy_bandwidth_gbps", "emit_gather_same_output_size")})))


if __name__ == "__main__":
    main()
