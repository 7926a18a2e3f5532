"""MAP: reads per second of dbgk_map_reads at the scale of the reference's E. coli test -- 250-base reads with 1 %
substitutions on about 5 Mb of contigs, k = 31, s = 5, both modes (map_reads: second alignment on, map_pair: off) -- for
several chunk ramps of the seed scan (dbgk_map_set_ramp).  Device time comes from the library's own events around each
kernel; the reads of a batch are already in host memory, the host-to-device copy is not part of the kernel figures.

    python profiles/measure_map.py [--reads 10000000] [--batch 1000000] [--ramps 4,8,16,64] [--out profiles/map_measure.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--batch", type=int, default=1000000)
    ap.add_argument("--ramps", default="4,8,16,64")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    genome = 5000000
    # contigs: a random 5 Mb genome cut into 100 adjacent pieces of 50 kb
    rng = np.random.default_rng(1)
    whole = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, genome)].tobytes()
    contigs = [whole[i:i + 50000] for i in range(0, len(whole), 50000)]
    # reads: 250-base windows of the same piece of the genome with 1 % substitutions, every second one reverse-complemented
    src = np.frombuffer(whole, dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y

    def make_batch(n):
        start = rng.integers(0, len(src) - 250, n)
        reads = src[start[:, None] + np.arange(250)[None, :]].copy()
        err = rng.random(reads.shape) < 0.01
        reads[err] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(err.sum()))]
        reads[1::2] = comp[reads[1::2, ::-1]]
        return reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * 250

    n_batches = max(1, a.reads // a.batch)
    batches = [make_batch(a.batch) for _ in range(min(n_batches, 2))]  # two distinct batches, alternated
    res = {"reads": n_batches * a.batch, "read_len": 250, "contig_bases": len(whole), "k": 31, "s": 5, "runs": []}
    for second in (True, False):
        with capi.Mapper(k=31, s=5, r=250, identity=0.97, second_alignment=second) as m:
            m.set_contigs(contigs)
            m.map(*batches[0])  # warm-up: buffers, identity table
            for ramp in [int(v) for v in a.ramps.split(",")]:
                m.set_ramp(ramp)
                ms = ms_long = 0.0
                windows = mapped = 0
                t0 = time.perf_counter()
                for b in range(n_batches):
                    hits = m.map(*batches[b % len(batches)])
                    st = m.batch_stats()
                    ms += st["ms_map"]
                    ms_long += st["ms_long"]
                    windows += st["windows_probed"]
                    mapped += int((hits["contig"][:, 0] != -1).sum())
                wall = time.perf_counter() - t0
                n = n_batches * a.batch
                run = {"mode": "map_reads" if second else "map_pair", "first_chunk": ramp, "ms_k_map_reads": ms, "ms_k_map_reads_long": ms_long,
                       "reads_per_s_device": n / (ms / 1e3), "reads_per_s_call": n / wall, "windows_per_read": windows / n,
                       "mapped_fraction": mapped / n}
                print(json.dumps(run), flush=True)
                res["runs"].append(run)
    if a.out:
        runs = res.pop("runs")
        open(a.out, "w").write("{\n " + json.dumps(res)[1:-1] + ",\n \"runs\": [\n" + ",\n".join("  " + json.dumps(r) for r in runs) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
