"""correct_error_reads on the GPU at scale: N synthetic 150 bp reads (1 % substitutions, some N) at k = 17, the table
from a KFREQ handle (cutoff 2), corrected in batches of the reference's bufferNum (1 M reads).  Prints one JSON line:
device ms per kernel, reads/s over the kernels, and the share of reads each kernel finished.  Reported, not gated.

    python profiles/measure_correct.py [--reads 10000000] [--genome 5000000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--batch", type=int, default=1000000)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    from oracle import oracle_py as O
    k, cutoff = 17, 2
    P = O.synth_params(a.genome, 150, sub_rate=0.01, n_rate=0.002, cfg=11)
    tot = {"ms_classify": 0.0, "ms_correct": 0.0, "ms_overflow": 0.0, "by_classify": 0, "by_correct": 0, "by_overflow": 0,
           "node_limit_hits": 0}
    deleted = 0
    t0 = time.time()
    with capi.Graph(k=k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000, expected_kmers=a.batch * 134) as g:
        for first in range(0, a.reads, a.batch):
            bases, offsets = O.synth_reads(P, first, min(a.batch, a.reads - first))
            g.push_reads(bases, offsets)
        g.finalize()
        with capi.Corrector(k=k) as c:
            c.from_kfreq(g, cutoff)
            hifreq = c.table_stats()[1]
            for first in range(0, a.reads, a.batch):
                bases, offsets = O.synth_reads(P, first, min(a.batch, a.reads - first))
                _, rec = c.correct(bases, offsets)
                st = c.batch_stats()
                for key in tot:
                    tot[key] += st[key]
                deleted += int(rec["deleted"].sum())
    ms = tot["ms_classify"] + tot["ms_correct"] + tot["ms_overflow"]
    out = dict(reads=a.reads, read_len=150, k=k, genome=a.genome, cutoff=cutoff, hifreq=hifreq, deleted=deleted,
               device_ms=round(ms, 2), reads_per_s=round(a.reads / (ms / 1e3)), wall_s=round(time.time() - t0, 1))
    out.update({key: (round(v, 2) if isinstance(v, float) else v) for key, v in tot.items()})
    out.update({"share_" + p: round(tot["by_" + p] / a.reads, 4) for p in ("classify", "correct", "overflow")})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
