"""GPU steps of tests/test_clean_edges_gpu.py, each run in a child process of its own under a time limit:
    python tests/clean_edges_gpu_steps.py edges_adapter | edges_lowqual | edges_host
Every scenario of tests/clean_edge_cases.py through capi.Cleaner against the restatement (tests/clean_restatement.py): integers
field for field, error_sum as a bit pattern, the counters against what the construction says.  Prints one JSON line of findings;
exits non-zero on a mismatch."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_edge_cases as E  # noqa: E402
import clean_restatement as CR  # noqa: E402
from clean_gpu_steps import same_blocks  # noqa: E402

COUNTERS = ("reads", "by_lds", "by_global", "hits", "cells")


def lowqual_batch(capi, scn):
    bases, offsets = capi.concat_sequences([b for b, _ in scn.reads])
    quals, _ = capi.concat_sequences([q for _, q in scn.reads])
    return bases, quals, offsets


def check_adapter(c, capi, scn):
    """one batch through the handle: every field of every hit, and the counters -> the counters"""
    got = [tuple(h) for h in c.adapter(*capi.concat_sequences(scn.reads)).tolist()]
    want = E.restated(scn.name)
    assert len(got) == len(want) == len(scn.reads)
    bad = [(n, scn.expect[n]["cat"], got[n], want[n]) for n in range(len(got)) if got[n] != tuple(want[n])]
    assert not bad, (scn.name, len(bad), bad[:5])
    st = {k: v for k, v in c.batch_stats().items() if k in COUNTERS}
    assert st == dict(E.census(scn), hits=sum(h[0] >= 0 for h in want), cells=E.cells_of(scn, want)), (scn.name, st)
    return st


def check_lowqual(c, capi, scn):
    got = c.lowqual(*lowqual_batch(capi, scn), scn.cutoff, scn.shift).tolist()
    want = E.restated(scn.name)
    assert len(got) == len(want) == len(scn.reads)
    bad = [(n, scn.expect[n]["cat"], got[n], want[n]) for n in range(len(got)) if not same_blocks(got[n], want[n])]
    assert not bad, (scn.name, len(bad), bad[:5])
    return {"reads": len(got), "trimmed": sum(b[3] for b in got)}


def edges_adapter():
    from dbg_assembly_amd import capi
    res = {}
    with capi.Cleaner() as c:
        for scn in E.adapter_scenarios():
            c.set_adapters([s for _, s in scn.adapters], scn.cutoff)
            res[scn.name] = check_adapter(c, capi, scn)
    return res


def edges_lowqual():
    from dbg_assembly_amd import capi
    res = {}
    with capi.Cleaner() as c:
        for scn in E.lowqual_scenarios():
            res[scn.name] = check_lowqual(c, capi, scn)
    return res


def big_batch():
    """more than 1 MiB of bases: 1200 reads of 1000 bases, one in four with M at its tail, qualities with a low stretch"""
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads, quals = [], []
    for n in range(1200):
        s = letters[rng.integers(0, 4, 1000)].tobytes()
        q = np.full(1000, 33 + 40, dtype=np.uint8)
        if n % 4 == 0:
            s = s[:980] + E.M + s[994:]
        if n % 3 == 0:
            q[int(rng.integers(0, 990)):][:10] = 33 + 2
        reads.append(s)
        quals.append(q.tobytes())
    return reads, quals


def edges_host():
    """one handle through the branches of clean_ensure_batch, set_adapters and the error table; every result equals what a fresh
    handle gives for the same call, and the restatement where a scenario is the input"""
    from dbg_assembly_amd import capi
    small, smaller = E.scenario("tie_t3_lds"), E.scenario("blocks")
    big_reads, big_quals = big_batch()
    big = capi.concat_sequences(big_reads)
    big_q = capi.concat_sequences(big_quals)[0]
    assert big[0].size > 1 << 20 and sum(len(b) for b, _ in smaller.reads) < sum(len(r) for r in small.reads)
    lds_set, global_set = E.scenario("tie_t1_lds"), E.scenario("tie_t1_global")
    n33, n64 = E.scenario("N_shift33"), E.scenario("N_shift64")

    def fresh(call):
        with capi.Cleaner() as f:
            return call(f)

    def big_adapter(h):
        h.set_adapters([s for _, s in small.adapters], small.cutoff)
        out = h.adapter(*big)
        return out.tobytes(), {k: v for k, v in h.batch_stats().items() if k in COUNTERS}

    def big_lowqual(h):
        return h.lowqual(big[0], big_q, big[1], 0.001, 33).tobytes()

    res = {}
    with capi.Cleaner() as c:
        # 1. adapter() on a small batch: the batch buffers exist, the quality buffer does not
        c.set_adapters([s for _, s in small.adapters], small.cutoff)
        res["small"] = check_adapter(c, capi, small)
        # 2. lowqual() on a smaller batch: only the quality buffer is missing
        res["smaller"] = check_lowqual(c, capi, smaller)
        # 3. more than 1 MiB of bases: the buffers grow, first without and then with qualities
        got = c.adapter(*big)
        st = {k: v for k, v in c.batch_stats().items() if k in COUNTERS}
        assert (got.tobytes(), st) == fresh(big_adapter), "adapter() behind a regrown batch differs from a fresh handle"
        assert st["hits"] >= 300 and st["by_lds"] == 1200
        assert [tuple(h) for h in got.tolist()] == CR.align_many(big_reads, E.named_adapters(small), small.cutoff)
        got_q = c.lowqual(big[0], big_q, big[1], 0.001, 33)
        assert got_q.tobytes() == fresh(big_lowqual), "lowqual() behind a regrown batch differs from a fresh handle"
        table = CR.error_table(33)
        assert all(same_blocks(g, CR.lowqual_block(E.text(r), E.text(q), 0.001, 33, table)) for g, r, q in zip(got_q.tolist(), big_reads, big_quals))
        assert 0 < int(got_q["trimmed"].sum()) < 1200
        res["big"] = st
        # 4. a global-form set, then an LDS-form set
        for scn in (global_set, lds_set):
            c.set_adapters([s for _, s in scn.adapters], scn.cutoff)
            res[scn.name] = check_adapter(c, capi, scn)
        assert res["tie_t1_global"]["by_lds"] == 0 and res["tie_t1_lds"]["by_global"] == 0
        # 5. quality shift 33, 64, 33
        for scn in (n33, n64, n33):
            res[scn.name] = check_lowqual(c, capi, scn)
        # and the small batch again, behind all of it
        c.set_adapters([s for _, s in small.adapters], small.cutoff)
        assert check_adapter(c, capi, small) == res["small"]
    return res


if __name__ == "__main__":
    print(json.dumps({"edges_adapter": edges_adapter, "edges_lowqual": edges_lowqual, "edges_host": edges_host}[sys.argv[1]]()))
