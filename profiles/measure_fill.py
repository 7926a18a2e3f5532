"""Measure link_contig on the GPU: a generated job of 10 M records over 10^6 contigs through capi.GapFiller with pageable buffers.
Writes profiles/fill_measure.json: per-stage device times (dbgk_fill_timing), the C-call rate of add_records, wall times of build,
resolve and emit.  Three runs, the first is warm-up; the figures are the median of the rest.

    python profiles/measure_fill.py [--records N] [--contigs N] [--reference /path/to/link_contig --reference-records N]

With --reference the shipped reference program is timed (wall) on a scaled-down copy of the job written as files; the JSON says
that the two sizes differ.  Without a GPU the file lists the figures that are missing."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fill_gpu_steps import large_job  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "fill_measure.json")
FIGURES = ("ms_orient", "ms_sort", "ms_table", "ms_gapstat", "ms_consensus", "ms_emit", "records_per_s_c_calls")


def gpu_runs(n_contigs, n, runs=3):
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(1)
    lens, recs, reads = large_job(rng, n_contigs, n, 200000, 128)
    contigs = [bytes(rng.integers(65, 66, int(x), dtype=np.uint8)) for x in lens]
    cbases, coff = capi.concat_sequences(contigs)
    rbases, roff = capi.concat_sequences([r.encode() for r in reads])
    r32 = np.zeros(len(recs), dtype=capi.FILL_RECORD_DTYPE)
    for f in capi.FILL_RECORD_DTYPE.names[:8]:
        r32[f] = recs[f]
    rows = []
    for _ in range(runs):
        with capi.GapFiller(3) as g:
            g.set_contigs(lens)
            g.set_reads((rbases, roff))
            t0 = time.perf_counter()
            for a in range(0, n, 1 << 22):
                g.add_records(r32[a:a + (1 << 22)])
            t_add = time.perf_counter() - t0
            t0 = time.perf_counter()
            g.build()
            t_build = time.perf_counter() - t0
            t0 = time.perf_counter()
            summ = g.resolve()
            t_resolve = time.perf_counter() - t0
            _, items, _, _, _ = g.layout()
            t0 = time.perf_counter()
            seq = g.emit((cbases, coff), items)
            t_emit = time.perf_counter() - t0
            st = g.timing()
        rows.append(dict(st, s_add_records=t_add, s_build=t_build, s_resolve=t_resolve, s_emit_call=t_emit,
                         records_per_s_c_calls=n / t_add, emitted=len(seq), **{"summary_" + k: v for k, v in summ.items()}))
    med = {k: statistics.median(r[k] for r in rows[1:]) for k in rows[0]}
    return med, rows


def reference_run(prog, n_contigs, n):
    """the reference program's wall time on a scaled-down copy of the job, written as the files it reads"""
    import gzip
    rng = np.random.default_rng(1)
    lens, recs, reads = large_job(rng, n_contigs, n, 20000, 128)
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "c.fa"), "w") as f:
        for c, x in enumerate(lens.tolist()):
            f.write(">ctg_%d\n%s\n" % (2 * c + 1, "A" * x))
    with gzip.open(os.path.join(d, "m.2ctg.gz"), "wt") as f:
        for r in recs.tolist():
            f.write("r%d\t%d\t1\t%d\tctg_%d\t1\t1\t1\t%s\t100%%\tr%d\t%d\t%d\t128\tctg_%d\t1\t1\t1\t%s\t100%%\n" % (
                r[0], r[1], r[2], 2 * r[4] + 1, chr(r[6]), r[0], r[1], r[3], 2 * r[5] + 1, chr(r[7])))
    with gzip.open(os.path.join(d, "m.2ctg.gz.reads.fa.gz"), "wt") as f:
        for k, q in enumerate(reads):
            f.write(">r%d\n%s\n" % (k, q))
    open(os.path.join(d, "m.lib"), "w").write("m.2ctg.gz\n")
    t0 = time.perf_counter()
    r = subprocess.run([prog, "-o", "ref", "c.fa", "m.lib"], cwd=d, capture_output=True)
    return {"wall_s": time.perf_counter() - t0, "returncode": r.returncode, "records": n, "contigs": n_contigs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000000)
    ap.add_argument("--contigs", type=int, default=1000000)
    ap.add_argument("--reference")
    ap.add_argument("--reference-records", type=int, default=1000000)
    a = ap.parse_args()
    res = {"job": {"records": a.records, "contigs": a.contigs, "buffers": "pageable"}}
    from dbg_assembly_amd import capi
    if capi.lib().dbgk_device_count() > 0:
        res["median_of_runs_2_and_3"], res["runs"] = gpu_runs(a.contigs, a.records)
    else:
        res["missing"] = list(FIGURES)
        res["note"] = "no GPU on the machine this file was written on: the GPU figures are not measured"
    if a.reference:
        res["reference"] = reference_run(a.reference, a.contigs * a.reference_records // a.records, a.reference_records)
        res["reference"]["note"] = "the reference ran a scaled-down copy of the job: the two sizes differ"
    else:
        res.setdefault("missing", []).append("reference wall time")
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res.get("median_of_runs_2_and_3", res)))


if __name__ == "__main__":
    main()
