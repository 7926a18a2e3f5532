"""GPU steps of tests/test_correct_gpu.py, each run in a child process of its own under a time limit:
    python tests/correct_gpu_steps.py capi_goldens | routes | edges_small | edges_chunks | edges_k19
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


# ---- the edge scenarios (tests/correct_edge_cases.py) ---------------------------------------------------------------------------
FIELDS = ("one_base", "tree", "deleted", "left_trim", "right_trim", "node_limit_hits", "path")


def edge_table(c, s, meta):
    """the scenario's table: the committed file where there is one, else its 4 KiB blocks that hold a bit, then the mirror"""
    if meta is not None and meta["table"]:
        c.load_file(os.path.join(GOLDEN, "correct_edges", meta["table"]))
    else:
        for at, blk in s.table.raw_blocks():
            c.load_bits(at, blk)
        c.seal()
    assert c.table_stats() == (4 ** s.k, s.table.n_canonical()), (s.name, c.table_stats())


def per_read(out, offsets, rec):
    return [(out[int(offsets[i]):int(offsets[i + 1])].tobytes(),) + tuple(int(rec[i][f]) for f in FIELDS) for i in range(len(rec))]


def want_of(r):
    return (r["out"], r["one_base"], r["tree"], r["deleted"], r["lt"], r["rt"], r["hits"], r["path"])


def edge_scenario(capi, s, meta, also=None):
    """one scenario through capi.Corrector: every read's bytes and every field of its record against the restatement, the
    pinned ones' .correct.fa text against the reference's committed bytes, and the batch counters against the expected paths"""
    import correct_edge_cases as E
    import gzip
    want = [want_of(r) for r in E.restated(s.name)]
    bases, offsets = pack(s.reads)
    with capi.Corrector(k=s.k, **s.opts) as c:
        edge_table(c, s, meta)
        out, rec = c.correct(bases, offsets)
        st = c.batch_stats()
        extra = also(c, out, rec) if also else None
    got = per_read(out, offsets, rec)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (s.name, bad[:10], [(got[i][1:], want[i][1:]) for i in bad[:3]])
    if s.pinned:
        recs = list(zip(E.headers(s), s.reads))
        assert records_to_file(recs, offsets, out, rec) == gzip.open(os.path.join(GOLDEN, "correct_edges", s.name + ".correct.fa.gz"), "rb").read(), s.name
        assert int(rec["node_limit_hits"].sum()) == meta["node_limit_hits"]
    paths = [w[-1] for w in want]
    assert (st["by_classify"], st["by_correct"], st["by_overflow"]) == (paths.count(0), paths.count(1), paths.count(2)), (s.name, st)
    assert st["node_limit_hits"] == sum(w[-2] for w in want) and st["reads"] == len(want)
    return {"reads": len(want), "paths": [paths.count(v) for v in (0, 1, 2)], "extra": extra}


def batch_shapes(s):
    """the mask_words scenario as 1, 3, 4 and 5 reads (classify packs four waves to a block), reversed, and again after a batch
    that held a 1025-base read (scratch and batch buffers are reused): every read's result is the one of the whole batch"""
    import correct_edge_cases as E

    def also(c, out, rec):
        def run(reads):
            b, o = pack(reads)
            got = c.correct(b, o)
            return per_read(got[0], o, got[1])
        whole = per_read(out, pack(s.reads)[1], rec)
        for n in (1, 3, 4, 5):
            assert run(s.reads[:n]) == whole[:n], n
        assert run(s.reads[::-1]) == whole[::-1]
        long_read = bytearray(s.genome[100:100 + E.LDS_READ_LEN + 1])
        long_read[1010] = E.other(long_read[1010], np.random.default_rng(1))
        want = want_of(E.restate_read(bytes(long_read), s.table, E.params_of(s)))
        assert want[-1] == 2 and run([bytes(long_read)]) == [want]
        assert c.batch_stats()["by_overflow"] == 1
        assert run(s.reads) == whole
        return "batch shapes 1/3/4/5, reversed, after a 1025-base read"
    return also


def edge_steps(pick):
    from dbg_assembly_amd import capi
    import correct_edge_cases as E
    meta = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "correct_edges", "cases.json")))}
    res = {}
    for s in E.scenarios():
        if pick(s):
            res[s.name] = edge_scenario(capi, s, meta.get(s.name), batch_shapes(s) if s.name == "mask_words" else None)
    return res


def edges_small():
    """k <= 13: reference-pinned but for k = 1 and the windows that start with a byte outside ACGTN (restatement only)"""
    return edge_steps(lambda s: s.k <= 13)


def edges_chunks():
    """k = 15, 16, 17: the tables go up as sparse blocks; the expected text is the reference's"""
    return edge_steps(lambda s: s.k in (15, 16, 17))


def edges_k19():
    """k = 19 against the restatement (parity unpinned), and seal() on word indices beyond 2^32"""
    import correct_edge_cases as E
    s = E.scenario("k19_parity_unpinned")
    T = s.table
    lo = min(T.canon)
    hi = max(v for v in T.canon if v >> 3 >= 1 << 32)
    assert lo >> 3 < 1 << 32

    def also(c, out, rec):
        for v in (lo, E.rcv(lo, s.k), hi, E.rcv(hi, s.k)):
            at = (v >> 15) * E.BLOCK
            assert np.array_equal(c.export_bits(at, E.BLOCK), T.raw_block(at, E.BLOCK, loaded=True)), v
        return [lo >> 3, hi >> 3]
    from dbg_assembly_amd import capi
    return {s.name: edge_scenario(capi, s, None, also)}


if __name__ == "__main__":
    print(json.dumps({"capi_goldens": capi_goldens, "routes": routes, "edges_small": edges_small, "edges_chunks": edges_chunks,
                      "edges_k19": edges_k19}[sys.argv[1]]()))
