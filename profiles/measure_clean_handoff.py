"""From raw reads with qualities to a k = 17 frequency table of the CLEANED reads, two routes on the same binary (10 M x 150 bp in
batches of 1 M reads; clean_lowqual -e 0.001 -q 33 -r 75, then clean_adapter with one contaminant, -s 12 -r 75):

  (a) today's route   per batch dbgk_clean_lowqual (upload of both planes, download of the blocks), the host cut, dbgk_clean_adapter
                      (second upload), the host cut, dbgk_push_reads into KFREQ (third upload)
  (b) the new route   per batch ONE upload of both planes; dbgk_clean_lowqual_device, dbgk_clean_compact, dbgk_clean_adapter_device
                      on the first handle's compact planes, dbgk_clean_compact, dbgk_push_cleaned into KFREQ

Each route runs --reps times, interleaved.  Reported:
  1. the device time of the length kernel + scan and of the gather, per stage, summed over the batches of a run;
  2. the gather's rate (bytes read + bytes written, both planes, per second of k_emit_gather) next to dbgk_measure_copy_bandwidth
     of the same run and next to k_emit_gather_lds (one plane, the corrector's gather) on a batch of the same output size -- the
     first batch, its reads cut to the lengths the two stages left.  (Its JSON key names that kernel as it was called when the first
     result file was written, k_corr_gather, so that old and new result files compare);
  3. the wall time of each route and of its stages (creating the handles is a stage of its own, the same work in both routes, and
     is left out of the comparison).  The project's rule decides whether the routes separate: the slowest run of the new route
     against the fastest of the old.  The host cut of route (a) is a numpy stand-in for the loops of bin/clean_lowqual and
     bin/clean_adapter, so the verdict is also given with the cut charged nothing.
Writes profiles/clean_handoff_measure.json; without a GPU it lists the figures that are missing.  Reported, not gated.

    python profiles/measure_clean_handoff.py [--reads 10000000] [--genome 5000000] [--reps 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "clean_handoff_measure.json")
FIGURES = ["ms_scan and ms_gather of both stages (3 runs)", "gather GB/s (bytes read + written, two planes)",
           "copy_bandwidth GB/s of the same run", "k_emit_gather_lds GB/s on a batch of the same output size",
           "route_a wall_s (3 runs)", "route_b wall_s (3 runs)", "routes_separate"]
K_FREQ, READ_LEN, MIN_LEN, SHIFT, CUTOFF_E, SCORE = 17, 150, 75, 33, 0.001, 12
ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"


def make_batch(O, P, first, n, seed):
    """n generator reads; one in six ends in the contaminant and random bases behind it, one in six has a Q2 tail, the rest is Q40"""
    bases, offsets = O.synth_reads(P, first, n)
    rng = np.random.default_rng(seed)
    reads = bases.reshape(n, READ_LEN).copy()
    quals = np.full((n, READ_LEN), SHIFT + 40, dtype=np.uint8)
    ad = np.frombuffer(ADAPTER.encode(), dtype=np.uint8)
    rows = np.arange(1, n, 6)
    cut = rng.integers(10, READ_LEN - len(ad), len(rows))
    junk = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (len(rows), READ_LEN))]
    col = np.arange(READ_LEN)[None, :]
    behind = col >= (cut + len(ad))[:, None]
    sub = reads[rows]
    sub[behind] = junk[behind]
    for j in range(len(ad)):
        sub[np.arange(len(rows)), cut + j] = ad[j]
    reads[rows] = sub
    rows = np.arange(4, n, 6)
    tail = rng.integers(10, 140, len(rows))
    q = quals[rows]
    q[col >= (READ_LEN - tail)[:, None]] = SHIFT + 2
    quals[rows] = q
    return reads.reshape(-1), quals.reshape(-1), offsets


def cut_lowqual(bases, quals, blocks):
    """the loop of bin/clean_lowqual (host/clean_lowqual.cpp:85-117) without its text, all reads READ_LEN long: a numpy stand-in"""
    n = len(blocks)
    quals = quals.copy()
    quals[bases == ord("N")] = SHIFT
    trimmed = blocks["trimmed"] != 0
    start = np.where(trimmed, np.maximum(blocks["start"] - 1, 0), 0).astype(np.int32)
    m = np.where(trimmed, np.where(blocks["start"] >= 1, blocks["length"], 0), READ_LEN).astype(np.int32)
    m[m < MIN_LEN] = 0
    col = np.arange(READ_LEN, dtype=np.int32)[None, :]
    keep = (col >= start[:, None]) & (col < (start + m)[:, None])
    coff = np.zeros(n + 1, dtype=np.uint64)
    coff[1:] = np.cumsum(m)
    return bases.reshape(n, READ_LEN)[keep], quals.reshape(n, READ_LEN)[keep], coff


def cut_adapter(bases, quals, offsets, hits):
    """the loop of bin/clean_adapter (host/clean_adapter.cpp:152-177) without its text: every read keeps a prefix"""
    lens = np.diff(offsets.astype(np.int64))
    m = np.where(hits["adapter"] >= 0, hits["read_start"] - 1, lens)
    m[m < MIN_LEN] = 0
    total = int(offsets[-1])
    delta = np.zeros(total + 1, dtype=np.int32)
    cutr = np.flatnonzero(m < lens)
    np.add.at(delta, offsets[:-1].astype(np.int64)[cutr] + m[cutr], 1)
    np.add.at(delta, offsets[1:].astype(np.int64)[cutr], -1)
    keep = np.cumsum(delta[:-1]) == 0
    coff = np.zeros(len(m) + 1, dtype=np.uint64)
    coff[1:] = np.cumsum(m)
    return bases[keep], quals[keep], coff


def kfreq(capi, batch):
    return capi.Graph(k=K_FREQ, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000, expected_kmers=batch * (READ_LEN - K_FREQ + 1))


def cleaners(capi):
    low, ad = capi.Cleaner(), capi.Cleaner()
    ad.set_adapters([ADAPTER], SCORE)
    return low, ad


def route_a(capi, batches):
    t = {"create": 0.0, "lowqual": 0.0, "cut_lowqual": 0.0, "adapter": 0.0, "cut_adapter": 0.0, "push": 0.0, "finalize": 0.0}
    t0 = time.perf_counter()
    low, ad = cleaners(capi)
    with kfreq(capi, len(batches[0][2]) - 1) as kf:
        t["create"] = time.perf_counter() - t0
        for bases, quals, offsets in batches:
            t1 = time.perf_counter()
            blocks = low.lowqual(bases, quals, offsets, CUTOFF_E, SHIFT)
            t2 = time.perf_counter()
            b1, q1, o1 = cut_lowqual(bases, quals, blocks)
            t3 = time.perf_counter()
            hits = ad.adapter(b1, o1)
            t4 = time.perf_counter()
            b2, _, o2 = cut_adapter(b1, q1, o1, hits)
            t5 = time.perf_counter()
            kf.push_reads(b2, o2)
            t6 = time.perf_counter()
            for name, dt in (("lowqual", t2 - t1), ("cut_lowqual", t3 - t2), ("adapter", t4 - t3), ("cut_adapter", t5 - t4), ("push", t6 - t5)):
                t[name] += dt
        t1 = time.perf_counter()
        st = kf.finalize()
        t["finalize"] = time.perf_counter() - t1
        wall = time.perf_counter() - t0
        spectrum = kf.kfreq_spectrum()[:8].tolist()
    low.close()
    ad.close()
    return {"wall_s": wall, "route_s": wall - t["create"], "stages_s": t, "kmers": int(st.total_kmers), "spectrum_head": spectrum}


def compact_offsets(capi, cleaner, n):
    off = np.empty(n + 1, dtype=np.uint64)
    assert capi.lib().dbgk_clean_compact_results(cleaner._h, None, None, off.ctypes.data) == 0
    return off


def route_b(capi, batches):
    t = {"create": 0.0, "upload": 0.0, "lowqual": 0.0, "compact_lowqual": 0.0, "adapter": 0.0, "compact_adapter": 0.0, "push": 0.0, "finalize": 0.0}
    ms = {"lowqual": [0.0, 0.0], "adapter": [0.0, 0.0]}
    moved = {"lowqual": 0, "adapter": 0}
    t0 = time.perf_counter()
    low, ad = cleaners(capi)
    with kfreq(capi, len(batches[0][2]) - 1) as kf:
        t["create"] = time.perf_counter() - t0
        for bases, quals, offsets in batches:
            n = len(offsets) - 1
            t1 = time.perf_counter()
            d_b, d_q = kf.malloc(bases.size + 64), kf.malloc(quals.size + 64)
            d_b.from_host(bases)
            d_q.from_host(quals)
            t2 = time.perf_counter()
            low.lowqual_device(d_b.ptr, d_q.ptr, offsets, CUTOFF_E, SHIFT)
            t3 = time.perf_counter()
            i1 = low.compact(MIN_LEN)
            p_b, p_q, _, _, _ = low.compact_device()
            o1 = compact_offsets(capi, low, n)
            t4 = time.perf_counter()
            ad.adapter_device(p_b, p_q, o1)
            t5 = time.perf_counter()
            i2 = ad.compact(MIN_LEN)
            t6 = time.perf_counter()
            kf.push_cleaned(ad)
            t7 = time.perf_counter()
            kf.sync()   # the caller's planes are freed below: nothing of this batch may still be queued
            d_b.free()
            d_q.free()
            for name, dt in (("upload", t2 - t1), ("lowqual", t3 - t2), ("compact_lowqual", t4 - t3), ("adapter", t5 - t4),
                             ("compact_adapter", t6 - t5), ("push", t7 - t6)):
                t[name] += dt
            for name, info in (("lowqual", i1), ("adapter", i2)):
                ms[name][0] += info["ms_scan"]
                ms[name][1] += info["ms_gather"]
                moved[name] += 2 * (info["clean_bases"] + (info["clean_bases"] + 15) // 16 * 16)
        t1 = time.perf_counter()
        st = kf.finalize()
        t["finalize"] = time.perf_counter() - t1
        wall = time.perf_counter() - t0
        spectrum = kf.kfreq_spectrum()[:8].tolist()
    low.close()
    ad.close()
    gbps = {k: moved[k] / (ms[k][1] * 1e6) if ms[k][1] else None for k in ms}
    return {"wall_s": wall, "route_s": wall - t["create"], "stages_s": t, "kmers": int(st.total_kmers), "spectrum_head": spectrum,
            "ms_scan": {k: v[0] for k, v in ms.items()}, "ms_gather": {k: v[1] for k, v in ms.items()}, "gather_bytes": moved, "gather_gbps": gbps}


def corr_gather_same_size(capi, batch):
    """k_emit_gather_lds on the first batch, its reads cut to the lengths the two cleaning stages leave: one plane of the same output
    size as the adapter stage's compact batch -> (GB/s of bytes read + written, ms, output bytes)"""
    bases, quals, offsets = batch
    n = len(offsets) - 1
    low, ad = cleaners(capi)
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        d_b, d_q = g.malloc(bases.size + 64), g.malloc(quals.size + 64)
        d_b.from_host(bases)
        d_q.from_host(quals)
        low.lowqual_device(d_b.ptr, d_q.ptr, offsets, CUTOFF_E, SHIFT)
        low.compact(MIN_LEN)
        p_b, p_q, _, _, _ = low.compact_device()
        ad.adapter_device(p_b, p_q, compact_offsets(capi, low, n))
        ad.compact(MIN_LEN)
        m = np.diff(compact_offsets(capi, ad, n).astype(np.int64))
        d_b.free()
        d_q.free()
    low.close()
    ad.close()
    rec = np.zeros(n, dtype=capi.CORR_REC_DTYPE)
    rec["right_trim"] = READ_LEN - m
    rec["deleted"] = m == 0
    best = None
    with capi.Corrector(k=9) as c:
        for _ in range(3):
            info = c.compact_from(bases, offsets, rec)
            assert info["result_bases"] == int(m.sum())
            best = info["ms_gather"] if best is None else min(best, info["ms_gather"])
    total = int(m.sum())
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
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--batch", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    job = dict(reads=a.reads, read_len=READ_LEN, genome=a.genome, batch=a.batch, k_kfreq=K_FREQ, min_len=MIN_LEN, error_rate_cutoff=CUTOFF_E,
               quality_shift=SHIFT, score_cutoff=SCORE, reps=a.reps)
    if capi.lib().dbgk_device_count() < 1:
        with open(a.out, "w") as f:
            json.dump({"job": job, "missing": FIGURES, "note": "no GPU on the machine this file was written on: nothing here is measured"}, f, indent=1)
            f.write("\n")
        print("no GPU: wrote the list of missing figures to", a.out)
        return
    from oracle import oracle_py as O
    P = O.synth_params(a.genome, READ_LEN, sub_rate=0.01, n_rate=0.002, cfg=11)
    batches = [make_batch(O, P, first, min(a.batch, a.reads - first), first) for first in range(0, a.reads, a.batch)]
    runs_a, runs_b = [], []
    for _ in range(a.reps):   # interleaved, so that a drift of the machine meets both routes
        runs_a.append(route_a(capi, batches))
        runs_b.append(route_b(capi, batches))
    assert len({(r["kmers"], tuple(r["spectrum_head"])) for r in runs_a + runs_b}) == 1, "the two routes counted different k-mers"
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:   # (any handle: the call needs a stream)
        copy_gbps = g.copy_bandwidth(2 << 30, 5)
    corr_gbps, corr_ms, corr_bytes = corr_gather_same_size(capi, batches[0])
    fast_a, slow_b = min(r["route_s"] for r in runs_a), max(r["route_s"] for r in runs_b)
    fast_a_no_cut = min(r["route_s"] - r["stages_s"]["cut_lowqual"] - r["stages_s"]["cut_adapter"] for r in runs_a)
    out = {"job": job, "route_a_today": runs_a, "route_b_device": runs_b,
           "rule": ("the slowest run of the new route against the fastest run of the old; compared is route_s = wall time without the "
                    "creation of the handles (stage `create`: identical work in both routes, 16 GiB of counters)"),
           "fastest_a_s": fast_a, "slowest_b_s": slow_b, "routes_separate": bool(slow_b < fast_a), "speedup_slowest_b_vs_fastest_a": fast_a / slow_b,
           "fastest_a_without_host_cut_s": fast_a_no_cut, "routes_separate_without_host_cut": bool(slow_b < fast_a_no_cut),
           "routes_separate_caveat": ("route (a)'s two cut stages are numpy stand-ins for the C++ loops of bin/clean_lowqual and "
                                      "bin/clean_adapter, not that code; routes_separate_without_host_cut charges route (a) nothing for them "
                                      "and is the verdict that does not depend on the stand-ins"),
           "gather_gbps": [r["gather_gbps"] for r in runs_b], "copy_bandwidth_gbps": copy_gbps,
           "gather_over_copy": [{k: (v / copy_gbps if v else None) for k, v in r["gather_gbps"].items()} for r in runs_b],
           "gather_bytes_counted": "per plane the kept bytes read and the 16-byte vectors written; two planes",
           "k_corr_gather_same_output_size": {"gbps": corr_gbps, "ms_gather_best_of_3": corr_ms, "output_bytes": corr_bytes,
                                              "note": "one plane, first batch, reads cut to the lengths both cleaning stages leave"},
           "gather_time": "ms_gather is the device time of k_emit_gather alone (events directly around the kernel)"}
    with open(a.out, "w") as f:
        json.dump(rounded(out), f, indent=1)
        f.write("\n")
    print(json.dumps(rounded({k: out[k] for k in ("fastest_a_s", "slowest_b_s", "routes_separate", "routes_separate_without_host_cut",
                                                  "gather_gbps", "copy_bandwidth_gbps", "k_corr_gather_same_output_size")})))


if __name__ == "__main__":
    main()
