"""CLEAN: reads per second of dbgk_clean_adapter and dbgk_clean_lowqual on 150-base synthetic reads, one in ten with an adapter
prefix at its tail: against the two default adapters (33 and 32 bases, cutoff 12), and against a set of 20 contaminants of 30 to 60
bases on both strands (40 sequences).  Device time comes from the library's own events around each kernel; "call" is the wall time
of the C call with pageable host buffers (copies in, kernel, copy out).  For clean_lowqual the bytes the kernel moves (bases and
qualities in, one 24-byte block per read out) over its device time stand next to the library's copy bandwidth.

    python profiles/measure_clean.py [--reads 10000000] [--batch 1000000] [--repeats 3] [--out profiles/clean_measure.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dbg_assembly_amd import capi  # noqa: E402

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
DEFAULT_ADAPTERS = ["GATCGGAAGAGCACACGTCTGAACTCCAGTCAC", "GATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"]


def reverse_complement(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--batch", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    contaminants = [LETTERS[rng.integers(0, 4, int(n))].tobytes().decode() for n in rng.integers(30, 61, 20)]
    sets = {"default_adapters": (DEFAULT_ADAPTERS, 12),
            "contaminants_20_both_strands": ([s for c in contaminants for s in (c, reverse_complement(c))], 12)}
    L = 150

    def make_batch(n, adapters):
        reads = LETTERS[rng.integers(0, 4, (n, L))]
        for row in range(0, n, 10):
            ad = np.frombuffer(adapters[row // 10 % len(adapters)].encode(), dtype=np.uint8)
            ad = ad[:int(rng.integers(12, len(ad) + 1))]
            reads[row, L - len(ad):] = ad
        quals = (33 + rng.choice([41, 40, 37, 30, 20, 2], (n, L), p=[.4, .3, .15, .08, .05, .02])).astype(np.uint8)
        return reads.reshape(-1), quals.reshape(-1), np.arange(n + 1, dtype=np.uint64) * L

    n_batches = max(1, a.reads // a.batch)
    n = n_batches * a.batch
    res = {"reads": n, "read_len": L, "batch": a.batch, "repeats": a.repeats, "runs": []}
    with capi.Cleaner() as c:
        for name, (adapters, cutoff) in sets.items():
            batches = [make_batch(a.batch, adapters) for _ in range(min(n_batches, 2))]  # two distinct batches, alternated
            c.set_adapters(adapters, cutoff)
            c.adapter(batches[0][0], batches[0][2])  # warm-up: buffers
            ms_runs, wall_runs = [], []
            for _ in range(a.repeats):
                ms, cells, hits = 0.0, 0, 0
                t0 = time.perf_counter()
                for b in range(n_batches):
                    bases, _, offsets = batches[b % len(batches)]
                    c.adapter(bases, offsets)
                    st = c.batch_stats()
                    ms += st["ms_lds"] + st["ms_global"]
                    cells += st["cells"]
                    hits += st["hits"]
                wall_runs.append(time.perf_counter() - t0)
                ms_runs.append(ms)
            ms, wall = statistics.median(ms_runs), statistics.median(wall_runs)
            run = {"kernel": "k_clean_adapter", "set": name, "sequences": len(adapters), "adapter_bases": sum(len(s) for s in adapters),
                   "ms_device": ms, "ms_device_min_max": [min(ms_runs), max(ms_runs)], "reads_per_s_device": n / (ms / 1e3),
                   "cell_updates_per_s_device": cells / (ms / 1e3), "s_call": wall, "reads_per_s_call": n / wall, "hit_fraction": hits / n}
            print(json.dumps(run), flush=True)
            res["runs"].append(run)
        c.lowqual(batches[0][0], batches[0][1], batches[0][2])
        ms_runs, wall_runs = [], []
        for _ in range(a.repeats):
            ms, trimmed = 0.0, 0
            t0 = time.perf_counter()
            for b in range(n_batches):
                bases, quals, offsets = batches[b % len(batches)]
                blocks = c.lowqual(bases, quals, offsets, 0.001, 33)
                ms += c.batch_stats()["ms_lowqual"]
                trimmed += int(blocks["trimmed"].sum())
            wall_runs.append(time.perf_counter() - t0)
            ms_runs.append(ms)
        ms, wall = statistics.median(ms_runs), statistics.median(wall_runs)
        moved = n * (2 * L + 8 + 24)
        run = {"kernel": "k_clean_lowqual", "ms_device": ms, "ms_device_min_max": [min(ms_runs), max(ms_runs)], "reads_per_s_device": n / (ms / 1e3),
               "bytes_moved": moved, "GBs_device": moved / (ms / 1e3) / 1e9, "s_call": wall, "reads_per_s_call": n / wall, "trimmed_fraction": trimmed / n}
        with capi.Graph(k=31, table_slots=capi.find_next_prime_ref(1000000), device=0) as g:
            run["copy_bandwidth_GBs"] = g.copy_bandwidth_detail(1 << 30, 5)[0]
        print(json.dumps(run), flush=True)
        res["runs"].append(run)
    res["reference_programs_t16_on_another_hosts_cpu"] = None  # context only; filled in by hand when it has been timed
    if a.out:
        runs = res.pop("runs")
        open(a.out, "w").write("{\n " + json.dumps(res)[1:-1] + ",\n \"runs\": [\n" + ",\n".join("  " + json.dumps(r) for r in runs) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
