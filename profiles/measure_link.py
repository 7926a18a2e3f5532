"""LINK: records per second of the link table build (dbgk_link_add_pairs + dbgk_link_build) on synthetic records over 10^6
contigs, and GB/s of dbgk_link_emit on a layout of about 1 Gb.  Device time comes from the library's own events around each
kernel (the two radix sorts are wall time around rocPRIM, their temporary buffers included); "call" is the wall time of the C calls
with pageable host buffers.  The emit figure (bytes written over kernel time) is to be read against the copy bandwidth
`bench.py --full` measures on the same box.  `--reference-seconds` records the wall time of the reference's own link_scaffold on
the text form of the same records, measured elsewhere: another machine's figure, kept apart.

    python profiles/measure_link.py [--records 10000000 100000000] [--contigs 1000000] [--emit-bases 1000000000] [--out profiles/link_measure.json]
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


def records(rng, lens, n):
    recs = np.zeros(n, dtype=capi.LINK_PAIR_DTYPE)
    c1 = rng.integers(0, len(lens), n)
    c2 = (c1 + rng.integers(1, 4, n)) % len(lens)
    recs["contig1"], recs["contig2"] = c1, c2
    for c, s, e in ((c1, "start1", "end1"), (c2, "start2", "end2")):
        recs[s] = (rng.random(n) * lens[c]).astype(np.int32) + 1
        recs[e] = np.minimum(recs[s] + 249, lens[c])
    d = np.frombuffer(b"FR", dtype=np.uint8)
    recs["direct1"], recs["direct2"] = d[rng.integers(0, 2, n)], d[rng.integers(0, 2, n)]
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[10000000, 100000000])
    ap.add_argument("--contigs", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=1 << 22)
    ap.add_argument("--emit-bases", type=int, default=1000000000)
    ap.add_argument("--reference-seconds", type=float, nargs="*", default=[])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    lens = rng.integers(200, 5000, a.contigs).astype(np.uint32)
    res = {"contigs": a.contigs, "batch": a.batch, "device": "one MI355X", "insert_size": 3000, "runs": []}
    for k, n in enumerate(a.records):
        recs = records(rng, lens, n)
        with capi.Scaffolder(0, 3, 3000) as s:
            s.set_contigs(lens)
            t0 = time.perf_counter()
            for p in range(0, n, a.batch):
                s.add_pairs(recs[p:p + a.batch])
            t1 = time.perf_counter()
            s.build()
            t2 = time.perf_counter()
            summ = s.resolve()
            t3 = time.perf_counter()
            st = s.batch_stats()
        run = {"records": n, "kept": st["kept"], "links": st["links"], "scaffolds": summ["scaffolds"],
               "ms_orient": st["ms_orient"], "ms_sort_wall": st["ms_sort"], "ms_reduce": st["ms_reduce"], "ms_chain": st["ms_chain"],
               "s_add_pairs_call": t1 - t0, "s_build_call": t2 - t1, "records_per_s_call": n / (t2 - t0),
               "s_host_passes_and_walk": t3 - t2,
               "reference_link_scaffold_wall_s_on_another_machine": a.reference_seconds[k] if k < len(a.reference_seconds) else None}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        del recs
    # emit: every contig once, every second one reversed, a gap of 100 between them
    n_ctg = max(1, a.emit_bases // 2600)
    offsets = np.zeros(n_ctg + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens[np.arange(n_ctg) % len(lens)].astype(np.uint64))
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(offsets[-1]))]
    items = np.zeros(2 * n_ctg, dtype=capi.LINK_ITEM_DTYPE)
    items["contig"][0::2], items["value"][0::2] = np.arange(n_ctg), np.arange(n_ctg) % 2
    items["contig"][1::2], items["value"][1::2] = -1, 100
    with capi.Scaffolder() as s:
        t0 = time.perf_counter()
        out = s.emit((bases, offsets), items)
        t1 = time.perf_counter()
        st = s.batch_stats()
    res["emit"] = {"bytes_out": int(len(out)), "items": int(len(items)), "ms_emit": st["ms_emit"], "s_call": t1 - t0,
                   "gb_per_s_written": len(out) / st["ms_emit"] / 1e6, "gb_per_s_read_and_written": 2 * len(out) / st["ms_emit"] / 1e6}
    print(json.dumps(res["emit"]), flush=True)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)
        open(a.out, "a").write("\n")


if __name__ == "__main__":
    main()
