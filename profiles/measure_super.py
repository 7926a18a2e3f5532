"""Measure link_supertig on the GPU: a generated job of 10^6 records over 10^5 contigs with 10 kb reads through capi.SuperLinker with
pageable buffers.  Writes profiles/super_measure.json: per-stage device times (dbgk_super_timing: orient, sorts, table,
k_super_gapstat, k_super_slices with the bytes it moved, emit), the C-call rate of add_records, wall times of build, resolve and
emit.  Three runs, the first is warm-up; the figures are the median of the rest.

    python profiles/measure_super.py [--records N] [--contigs N] [--read-len N]

The reference program is not timed.  Without a GPU the file lists the figures that are missing."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "super_measure.json")
FIGURES = ("ms_orient", "ms_sort", "ms_table", "ms_gapstat", "ms_slices", "slice_GB_per_s", "ms_emit", "records_per_s_c_calls")


def job(rng, n_contigs, n, n_reads, read_len):
    """chains of four contigs, ten records per junction on average, a tenth of the records anywhere; every slice lies in its read"""
    from dbg_assembly_amd import capi
    lens = rng.integers(2000, 6000, n_contigs).astype(np.uint32)
    recs = np.zeros(n, dtype=capi.FILL_RECORD_DTYPE)
    c1 = rng.integers(0, n_contigs - 4, n)
    c1 -= (c1 % 4 == 3)
    c2 = c1 + 1
    noise = rng.random(n) < 0.1
    c2[noise] = (c1[noise] + rng.integers(2, 50, int(noise.sum()))) % n_contigs
    gap = ((c1 * 2654435761) % 400).astype(np.int64) - 50 + rng.integers(-10, 11, n)
    recs["read"] = rng.integers(0, n_reads, n)
    recs["read_len"] = read_len
    recs["align1_end"] = rng.integers(1000, read_len - 2000, n)
    recs["align2_start"] = recs["align1_end"] + gap + 1
    swap = rng.random(n) < 0.5
    recs["contig1"], recs["contig2"] = np.where(swap, c2, c1), np.where(swap, c1, c2)
    recs["direct1"] = np.where(swap, ord("R"), ord("F"))
    recs["direct2"] = recs["direct1"]
    reads = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n_reads * read_len)]
    offsets = np.arange(n_reads + 1, dtype=np.uint64) * read_len
    return lens, recs, (reads, offsets)


def gpu_runs(n_contigs, n, read_len, runs=3):
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(1)
    lens, recs, reads = job(rng, n_contigs, n, 20000, read_len)
    cbases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(lens.sum()))]
    coff = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    rows = []
    for _ in range(runs):
        with capi.SuperLinker(3) as g:
            g.set_contigs(lens)
            g.set_reads(reads)
            t0 = time.perf_counter()
            for a in range(0, n, 1 << 22):
                g.add_records(recs[a:a + (1 << 22)])
            t_add = time.perf_counter() - t0
            t0 = time.perf_counter()
            g.build()
            t_build = time.perf_counter() - t0
            t0 = time.perf_counter()
            summ = g.resolve()
            t_resolve = time.perf_counter() - t0
            _, items, _, _ = g.layout()
            t0 = time.perf_counter()
            seq = g.emit((cbases, coff), items)
            t_emit = time.perf_counter() - t0
            st = g.timing()
        # the slice kernel reads and writes slice_bytes each
        rate = 2 * st["slice_bytes"] / (st["ms_slices"] * 1e6) if st["ms_slices"] else 0.0
        rows.append(dict(st, s_add_records=t_add, s_build=t_build, s_resolve=t_resolve, s_emit_call=t_emit, slice_GB_per_s=rate,
                         records_per_s_c_calls=n / t_add, emitted=len(seq), **{"summary_" + k: v for k, v in summ.items()}))
    med = {k: statistics.median(r[k] for r in rows[1:]) for k in rows[0]}
    return med, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1000000)
    ap.add_argument("--contigs", type=int, default=100000)
    ap.add_argument("--read-len", type=int, default=10000)
    a = ap.parse_args()
    res = {"job": {"records": a.records, "contigs": a.contigs, "read_len": a.read_len, "buffers": "pageable"}}
    from dbg_assembly_amd import capi
    if capi.lib().dbgk_device_count() > 0:
        res["median_of_runs_2_and_3"], res["runs"] = gpu_runs(a.contigs, a.records, a.read_len)
    else:
        res["missing"] = list(FIGURES)
        res["note"] = "no GPU on the machine this file was written on: the GPU figures are not measured"
    res.setdefault("missing", []).append("reference wall time (the reference program was not timed)")
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res.get("median_of_runs_2_and_3", res)))


if __name__ == "__main__":
    main()
