"""GPU steps of tests/test_correct_gpu.py, each run in a child process of its own under a time limit:
    python tests/correct_gpu_steps.py capi_goldens | routes
Prints one JSON line of findings; exits non-zero on a mismatch."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import correct_restatement as CR  # noqa: E402
from test_correct_cpu import GOLDEN, expected_fa, golden_cases, params_of  # noqa: E402


def records_to_file(recs, offsets, out, rec):
    """the .correct.fa text from the device results (what the command line writes, decompressed)"""
    return b"".join(CR.record_line(head, out[int(offsets[i]):int(offsets[i + 1])].tobytes(), int(q["one_base"]), int(q["tree"]),
                                   int(q["deleted"]), int(q["left_trim"]), int(q["right_trim"]))[0]
                    for i, ((head, _), q) in enumerate(zip(recs, rec)))


def pack(seqs):
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offsets


def capi_goldens():
    from dbg_assembly_amd import capi
    res = {}
    for d, case in golden_cases():
        P = params_of(case)
        recs = CR.read_records(os.path.join(GOLDEN, d, case["reads"]), case["format"])
        bases, offsets = pack([s for _, s in recs])
        with capi.Corrector(k=P.k, m=P.m, c=P.c, x=P.x, n=P.n, r=P.r) as c:
            c.load_file(os.path.join(GOLDEN, d, "table.cz"))
            assert c.table_stats() == (4 ** P.k, case["hifreq"]), (d, case["name"], c.table_stats())
            out, rec = c.correct(bases, offsets)
            st = c.batch_stats()
        got = records_to_file(recs, offsets, out, rec)
        assert got == expected_fa(d, case), (d, case["name"])
        assert int(rec["node_limit_hits"].sum()) == case["node_limit_hits"]
        assert st["by_classify"] + st["by_correct"] + st["by_overflow"] == len(recs)
        res["%s/%s" % (d, case["name"])] = {k: st[k] for k in ("by_classify", "by_correct", "by_overflow")}
    return res


class CanonTable(CR.Table):
    """lookups on a kmerfreq file's raw bits: the loaded bit of v is the raw bit of canonical(v)"""

    def __init__(self, raw, k):
        super().__init__(raw, k)
        self.k = k

    def hi(self, v):
        if v >= self.total:
            return False
        r, x = 0, v
        for _ in range(self.k):
            r = (r << 2) | (3 - (x & 3))
            x >>= 2
        return super().hi(min(v, r))


def routes():
    """route (b) (KFREQ handle + cutoff) equals route (a) (the raw bits kmerfreq -b 1 -m cutoff writes, loaded) at k = 17"""
    from dbg_assembly_amd import capi
    from oracle import oracle_py as O
    k, cutoff, n_reads = 17, 2, 200000
    bases, offsets = O.synth_reads(O.synth_params(1000000, 150, sub_rate=0.01, n_rate=0.002, cfg=7), 0, n_reads)
    with capi.Graph(k=k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000, expected_kmers=n_reads * 134) as g:
        g.push_reads(bases, offsets)
        g.finalize()
        raw = g.kfreq_bits(cutoff)
        with capi.Corrector(k=k) as b:
            b.from_kfreq(g, cutoff)
            out_b, rec_b = b.correct(bases, offsets)
            st_b = b.batch_stats()
            stats_b = b.table_stats()
            bits_b_head = b.export_bits(0, 1 << 24)
    with capi.Corrector(k=k) as a:
        step = 1 << 26
        for at in range(0, raw.size, step):
            a.load_bits(at, raw[at:at + step])
        a.seal()
        out_a, rec_a = a.correct(bases, offsets)
        stats_a = a.table_stats()
        bits_a_head = a.export_bits(0, 1 << 24)
    assert stats_a == stats_b, (stats_a, stats_b)
    assert np.array_equal(bits_a_head, bits_b_head)
    assert np.array_equal(out_a, out_b) and np.array_equal(rec_a, rec_b)
    # a 5 k-read sample against the restatement, on the handle's exported bits
    T = CanonTable(raw, k)
    P = CR.Params(k=k)
    rng = np.random.default_rng(5)
    diffs = 0
    for i in sorted(rng.choice(n_reads, 5000, replace=False)):
        o, e = int(offsets[i]), int(offsets[i + 1])
        read, one, multi, deleted, lt, rt, hits = CR.correct_one_read(bases[o:e].tobytes(), T, P)
        q = rec_b[i]
        same = (read == out_b[o:e].tobytes() and (one, multi, deleted, lt, rt, hits) ==
                (int(q["one_base"]), int(q["tree"]), int(q["deleted"]), int(q["left_trim"]), int(q["right_trim"]), int(q["node_limit_hits"])))
        diffs += not same
    assert diffs == 0, diffs
    return {"hifreq": stats_b[1], "by_classify": st_b["by_classify"], "by_correct": st_b["by_correct"],
            "by_overflow": st_b["by_overflow"], "ms": [st_b["ms_classify"], st_b["ms_correct"], st_b["ms_overflow"]],
            "deleted": int(rec_b["deleted"].sum()), "tree": int(rec_b["tree"].sum()), "one_base": int(rec_b["one_base"].sum())}


if __name__ == "__main__":
    print(json.dumps({"capi_goldens": capi_goldens, "routes": routes}[sys.argv[1]]()))
