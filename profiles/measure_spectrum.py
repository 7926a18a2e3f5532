#!/usr/bin/env python3
"""The two table scans of dbgk_spectrum.h at their stated sizes on one MI355X.  Reported, not gated: no threshold is set.

  k_kf_spectrum   the 4^17 byte counters (16 GiB) of 10 M x 150 bp synthetic reads (the cfg2 generator), binned whole:
                  device ms between two events around the kernel (dbgk_kfreq_spectrum_ms), best of 5, as GB/s read, next
                  to the copy bandwidth dbgk_measure_copy_bandwidth gives in the same run (bytes read + bytes written).
                  The wall time of the whole call is recorded beside it.
  k_mut_scan      a synthetic 100 Mb genome at k = 17, -s 100 (one million sites): device ms between two events around
                  the kernel (dbgk_corr_mutation_scan_ms), best of 3.

    python profiles/measure_spectrum.py [--reads 10000000] [--genome 100000000] [--out profiles/spectrum_measure.json]

Without a GPU the record is written all the same and says which figures are missing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dbg_assembly_amd import capi  # noqa: E402

K = 17


def measure_spectrum(g, n_reads, out):
    P = capi.synth_params(50_000_000, 150, cfg=2)
    d_bases, d_off, nb = g.synth_reads_device(P, 0, n_reads)
    g.push_reads_device(d_bases.ptr, d_off.ptr, n_reads, nb)
    st = g.finalize()
    d_bases.free()
    d_off.free()
    best, wall, hist = None, None, None
    for _ in range(5):
        t0 = time.perf_counter()
        hist = g.kfreq_spectrum()
        dt = time.perf_counter() - t0
        ms = g.kfreq_spectrum_ms()
        best = ms if best is None else min(best, ms)
        wall = dt if wall is None else min(wall, dt)
    assert int(hist[1:].sum()) == int(st.count) and int(hist.sum()) == 4 ** K
    out["spectrum"] = {"table_bytes": 4 ** K, "windows": int(st.stored_kmers), "species": int(st.count),
                       "zero_share": float(hist[0]) / 4 ** K, "kernel_ms_best_of_5": best, "GBps_read": 4 ** K / best / 1e6,
                       "call_ms_wall_best_of_5": wall * 1e3, "copy_bandwidth_GBps_read_plus_written": g.copy_bandwidth(2 << 30, 5)}


def measure_scan(g, genome_len, skip, out):
    rng = np.random.default_rng(17)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, genome_len)]
    piece, step = 1 << 20, (1 << 20) - (K - 1)    # every window once, as bin/simulate_lowfreq_kmer pushes a sequence
    starts = [s for s in range(0, genome_len, step) if s + K <= genome_len]
    parts = [genome[s:s + piece] for s in starts]
    offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in parts])
    g.reset()
    g.push_reads(np.concatenate(parts), offsets)
    st = g.finalize()
    assert int(st.stored_kmers) == genome_len - K + 1
    with capi.Corrector(k=K) as c:
        c.from_kfreq(g, 0)
        whole = np.array([0, genome_len], dtype=np.uint64)
        best, hist = None, None
        for _ in range(3):
            hist = c.mutation_scan(genome, whole, skip)
            ms = c.mutation_scan_ms()
            best = ms if best is None else min(best, ms)
    out["mutation_scan"] = {"genome": genome_len, "k": K, "skip": skip, "sites": int(hist.sum()), "hist": [int(v) for v in hist],
                            "kernel_ms_best_of_3": best, "M_sites_per_s": float(hist.sum()) / best / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--skip", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_measure.json"))
    a = ap.parse_args()
    out = {"job": {"k": K, "reads": a.reads, "read_length": 150, "genome": a.genome, "skip": a.skip}, "missing": []}
    try:
        with capi.Graph(k=K, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1 << 20, expected_kmers=a.reads * (150 - K + 1)) as g:
            for name, run in (("spectrum", lambda: measure_spectrum(g, a.reads, out)), ("mutation_scan", lambda: measure_scan(g, a.genome, a.skip, out))):
                try:
                    run()
                except (capi.DbgkError, AssertionError, MemoryError) as e:
                    out["missing"].append("%s: %s" % (name, e))
    except capi.DbgkError as e:
        out["missing"] += ["spectrum: " + str(e), "mutation_scan: " + str(e)]
    if out["missing"]:
        out["note"] = "the figures listed as missing have not been measured"
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
