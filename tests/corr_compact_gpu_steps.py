"""GPU steps of tests/test_corr_compact_gpu.py, each run in a child process of its own under a time limit:
    python tests/corr_compact_gpu_steps.py crafted | goldens | edges_small | edges_chunks | device_input | handoff | reuse | two_handles
Prints one JSON line of findings; exits non-zero on a mismatch."""
import ctypes
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import corr_compact_restatement as CC  # noqa: E402
import correct_restatement as CR  # noqa: E402
from correct_gpu_steps import edge_table, pack  # noqa: E402
from test_correct_cpu import GOLDEN, expected_fa, golden_cases, params_of  # noqa: E402

EDGES = os.path.join(GOLDEN, "correct_edges")


# ---- crafted batches through compact_from ------------------------------------------------------------------------------------------
def craft(rng, lens, lts, rts, deleted):
    """random bytes under the given lengths and trims; the other record fields are random too (they feed the counters)"""
    lens = np.asarray(lens, dtype=np.uint64)
    n = len(lens)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    bases = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    rec = np.zeros(n, dtype=CC.REC_DTYPE)
    rec["left_trim"], rec["right_trim"], rec["deleted"] = lts, rts, deleted
    rec["one_base"], rec["tree"] = rng.integers(0, 3, n), rng.integers(0, 3, n)
    rec["node_limit_hits"], rec["path"] = rng.integers(0, 2, n), rng.integers(0, 3, n)
    return bases, offsets, rec


def kept(rng, out_lens):
    """reads with the given OUTPUT lengths: random trims around them, none deleted"""
    out_lens = np.asarray(out_lens, dtype=np.int64)
    lts, rts = rng.integers(0, 20, len(out_lens)), rng.integers(0, 20, len(out_lens))
    return out_lens + lts + rts, lts, rts, np.zeros(len(out_lens), dtype=np.uint8)


def join(*parts):
    return tuple(np.concatenate([np.asarray(p[i]) for p in parts]) for i in range(4))


def zeros(n):
    """n deleted reads of 30 bytes"""
    return np.full(n, 30), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.uint8)


def with_total(rng, total):
    """short reads whose output lengths sum to `total` exactly"""
    lens = []
    while sum(lens) < total:
        lens.append(min(int(rng.integers(1, 101)), total - sum(lens)))
    return kept(rng, lens)


def pair_rows():
    """every pair (source start mod 4, destination start mod 4) at output lengths 1, 2, 3, 4, 5 and 17: in front of each target
    read an untrimmed read moves the destination (and the source), a deleted one the source alone; the target is trimmed by 2
    bytes on the left and 3 on the right -> (the case, target indices)"""
    rows, targets, src, dst = [], [], 0, 0
    for m in (1, 2, 3, 4, 5, 17):
        for s in range(4):
            for d in range(4):
                x = (d - dst) % 4 + 4
                rows.append((x, 0, 0, 0))
                src, dst = src + x, dst + x
                e = (s - src - 2) % 4
                rows.append((e, 0, 0, 1))
                src += e
                targets.append(len(rows))
                rows.append((2 + m + 3, 2, 3, 0))
                src, dst = src + 2 + m + 3, dst + m
    return tuple(np.array(col, dtype=t) for col, t in zip(zip(*rows), (np.int64, np.int64, np.int64, np.uint8))), targets


def crafted():
    from dbg_assembly_amd import capi
    T = capi.CORR_COMPACT_TILE
    rng = np.random.default_rng(20)
    cases = {}
    cases["n1"] = kept(rng, [37])
    cases["all_deleted"] = zeros(1000)
    lens = rng.integers(1, 101, 4000)
    lts = (rng.random(4000) * lens).astype(np.int64)
    rts = (rng.random(4000) * (lens - lts)).astype(np.int64)
    cases["lengths_1_100"] = (lens, lts, rts, (rng.random(4000) < 0.05).astype(np.uint8))
    for name, total in (("total_T", T), ("total_T_plus_1", T + 1), ("total_T_minus_1", T - 1), ("total_15", 15)):
        cases[name] = with_total(rng, total)
    cases["zero_run_3T_inside_a_tile"] = join(with_total(rng, T + 1000), zeros(3 * T), with_total(rng, 2 * T))
    cases["zero_run_on_a_tile_boundary"] = join(with_total(rng, 2 * T), zeros(3 * T), with_total(rng, T + 5))
    cases["zero_run_one_byte_past_a_boundary"] = join(with_total(rng, T + 1), zeros(3 * T), with_total(rng, 300))
    cases["zero_first_and_last"] = join(zeros(1), with_total(rng, 500), zeros(1))
    for a in (0, 5):   # the long read at two alignments of source and destination
        cases["long_read_spans_three_tiles_%d" % a] = join(kept(rng, [40 + a, 60]), kept(rng, [2 * T + 17]), kept(rng, [33, 80]))
    # left_trim + right_trim == L on a read that is kept, one that trims more than it holds, and a deleted read with trims
    cases["trims_use_up_the_read"] = join(kept(rng, [50]), (np.array([60, 60, 60]), np.array([25, 50, 10]), np.array([35, 30, 10]), np.array([0, 0, 1], dtype=np.uint8)),
                                          kept(rng, [70]))
    cases["source_and_destination_mod_4"] = pair_rows()[0]
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Corrector(k=9) as c:
        for name, (lens, lts, rts, dele) in cases.items():
            bases, offsets, rec = craft(rng, lens, lts, rts, dele)
            want_b, want_o, want_c = CC.compact(bases, offsets, rec)
            info = c.compact_from(bases, offsets, rec)
            got_b, got_o = c.compact_to_host()
            assert np.array_equal(got_o, want_o), name
            assert np.array_equal(got_b, want_b), (name, int(np.flatnonzero(got_b != want_b)[0]))
            assert {f: info[f] for f in CC.COUNTERS} == want_c, (name, info, want_c)
            d_b, d_o, n, nb = c.compact_device()
            assert (n, nb) == (len(lens), len(want_b)) and d_b % 16 == 0 and d_o % 8 == 0
            if nb % 16:   # the pad of the last vector
                tail = np.full(16, 0xAA, dtype=np.uint8)
                assert capi.lib().dbgk_memcpy_d2h(g._h, tail.ctypes.data, ctypes.c_void_p(d_b + nb - nb % 16), 16) == 0
                assert np.array_equal(tail[:nb % 16], want_b[nb - nb % 16:]) and not tail[nb % 16:].any(), name
            res[name] = {"reads": n, "bases": nb, "ms_gather": info["ms_gather"]}
            if name == "lengths_1_100":
                live = CC.out_lengths(offsets, rec) > 0
                src = (offsets[:-1][live] + rec["left_trim"][live].astype(np.uint64)) % np.uint64(16)
                dst = want_o[:-1][live] % np.uint64(16)
                assert set(src.tolist()) == set(range(16)) and set(dst.tolist()) == set(range(16))
                assert set((src * np.uint64(16) + dst).tolist()) == set(range(256))   # ... independently of each other
            if name == "source_and_destination_mod_4":
                seen = {((int(offsets[i]) + int(rec["left_trim"][i])) % 4, int(want_o[i]) % 4, int(want_o[i + 1] - want_o[i])) for i in pair_rows()[1]}
                assert seen == {(s, d, m) for s in range(4) for d in range(4) for m in (1, 2, 3, 4, 5, 17)}
            if name == "all_deleted":
                assert nb == 0 and info["deleted_reads"] == 1000 and info["ms_gather"] == 0
            if name == "trims_use_up_the_read":
                assert CC.out_lengths(offsets, rec).tolist()[1:4] == [0, 0, 0] and info["result_reads"] == 4
    return res


# ---- goldens: Corrector.correct, then compact() --------------------------------------------------------------------------------------
def check_golden(c, seqs, fa, stat_text, name):
    bases, offsets = pack(seqs)
    out, rec = c.correct(bases, offsets)
    info = c.compact()
    got_b, got_o = c.compact_to_host()
    assert CC.as_lines(got_b, got_o) == CC.sequence_lines(fa), name
    assert CC.stat_of(info, int(offsets[-1])) == CC.stat_numbers(stat_text), (name, info)
    want_b, want_o, want_c = CC.compact(out, offsets, rec)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_o, want_o) and {f: info[f] for f in CC.COUNTERS} == want_c, name
    st = c.batch_stats()
    assert (info["by_classify"], info["by_correct"], info["by_overflow"], info["node_limit_hits"]) == \
        (st["by_classify"], st["by_correct"], st["by_overflow"], st["node_limit_hits"]), name
    return {f: info[f] for f in ("reads", "result_reads", "deleted_reads", "trimmed_reads", "by_overflow")}


def goldens():
    from dbg_assembly_amd import capi
    res = {}
    for d, case in golden_cases():
        P = params_of(case)
        recs = CR.read_records(os.path.join(GOLDEN, d, case["reads"]), case["format"])
        with capi.Corrector(k=P.k, m=P.m, c=P.c, x=P.x, n=P.n, r=P.r) as c:
            c.load_file(os.path.join(GOLDEN, d, "table.cz"))
            res["%s/%s" % (d, case["name"])] = check_golden(c, [s for _, s in recs], expected_fa(d, case),
                                                            open(os.path.join(GOLDEN, d, case["name"] + ".correct.stat")).read(), case["name"])
    return res


def edges(pick):
    from dbg_assembly_amd import capi
    import correct_edge_cases as E
    meta = {c["name"]: c for c in json.load(open(os.path.join(EDGES, "cases.json")))}
    res = {}
    for s in E.scenarios():
        if s.pinned and pick(s):
            with capi.Corrector(k=s.k, **s.opts) as c:
                edge_table(c, s, meta[s.name])
                res[s.name] = check_golden(c, s.reads, gzip.open(os.path.join(EDGES, s.name + ".correct.fa.gz"), "rb").read(),
                                           open(os.path.join(EDGES, s.name + ".correct.stat")).read(), s.name)
    return res


def edges_small():
    return edges(lambda s: s.k <= 13)


def edges_chunks():
    return edges(lambda s: s.k > 13)


# ---- device input ----------------------------------------------------------------------------------------------------------------------
def device_input():
    """correct_device on a buffer the test uploaded == correct on the host copy: records, batch stats, compact batch"""
    from dbg_assembly_amd import capi
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        for d, name in (("correct_k9_dense", "n4000"), ("correct_k12", "default")):
            case = next(c for dd, c in golden_cases() if dd == d and c["name"] == name)
            P = params_of(case)
            bases, offsets = pack([s for _, s in CR.read_records(os.path.join(GOLDEN, d, case["reads"]), case["format"])])
            buf = g.malloc(bases.size + 64)
            buf.from_host(bases)
            with capi.Corrector(k=P.k, m=P.m, c=P.c, x=P.x, n=P.n, r=P.r) as c:
                c.load_file(os.path.join(GOLDEN, d, "table.cz"))
                out, rec_h = c.correct(bases, offsets)
                st_h, info_h = c.batch_stats(), c.compact()
                b_h, o_h = c.compact_to_host()
                rec_d = c.correct_device(buf.ptr, offsets)
                st_d, info_d = c.batch_stats(), c.compact()
                b_d, o_d = c.compact_to_host()
            assert np.array_equal(buf.to_host(np.uint8, bases.size), bases), "the caller's buffer was written"
            buf.free()
            counts = ("reads", "by_classify", "by_correct", "by_overflow", "node_limit_hits")
            assert np.array_equal(rec_d, rec_h) and [st_d[f] for f in counts] == [st_h[f] for f in counts], (d, name)
            assert np.array_equal(b_d, b_h) and np.array_equal(o_d, o_h) and all(info_d[f] == info_h[f] for f in CC.COUNTERS), (d, name)
            assert CC.as_lines(b_d, o_d) == CC.sequence_lines(expected_fa(d, case))
            res["%s/%s" % (d, name)] = {"by_overflow": st_d["by_overflow"], "reads": st_d["reads"]}
    assert res["correct_k9_dense/n4000"]["by_overflow"] > 0 and res["correct_k12/default"]["by_overflow"] == 0
    return res


# ---- hand-off to the graph ---------------------------------------------------------------------------------------------------------------
K_CORR, K_GRAPH, CUTOFF, READ_LEN = 13, 31, 2, 100


def workload(n_reads=30000, genome=40000):
    """100-bp reads with substitution errors from the generator of the `routes` step, and 1 % random reads among them"""
    from oracle import oracle_py as O
    bases, offsets = O.synth_reads(O.synth_params(genome, READ_LEN, sub_rate=0.01, n_rate=0.0, cfg=7), 0, n_reads)
    rng = np.random.default_rng(9)
    reads = bases.reshape(n_reads, READ_LEN).copy()
    junk = rng.choice(n_reads, n_reads // 100, replace=False)
    reads[junk] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (len(junk), READ_LEN))]
    return reads.reshape(-1), offsets


def host_trim(out, offsets, rec):
    """today's host route: the loop of host/correct_error_reads.cpp:151-174 -> the sequence lines, deleted reads empty"""
    seqs = []
    for i in range(len(rec)):
        o, e = int(offsets[i]), int(offsets[i + 1])
        seqs.append(b"" if rec[i]["deleted"] else out[o + int(rec[i]["left_trim"]):e - int(rec[i]["right_trim"])].tobytes())
    return seqs


def graph_args(engine, n_reads):
    from dbg_assembly_amd import capi
    if engine == "direct":
        return dict(k=K_GRAPH, table_slots=capi.find_next_prime_ref(4000000), engine=capi.ENGINE_DIRECT, max_read_len=250)
    return dict(k=K_GRAPH, table_slots=capi.find_next_prime_ref(70000000), engine=capi.ENGINE_PARTITION, max_read_len=250,
                expected_kmers=n_reads * (READ_LEN - K_GRAPH + 1))


def result_of(g):
    st = g.finalize()
    return (int(st.total_reads), int(st.total_kmers), int(st.count)), g.export_sorted(), bytes(g.link_stats())


def same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    assert a[2] == b[2], what


class Chain:
    """one upload; KFREQ from the resident reads; the corrector's table from KFREQ"""

    def __init__(self, capi, bases, offsets):
        self.capi, self.bases, self.offsets, n = capi, bases, offsets, len(offsets) - 1
        self.kf = capi.Graph(k=K_CORR, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000)
        self.d_b, self.d_o = self.kf.malloc(bases.size + 64), self.kf.malloc((n + 1) * 8)
        self.d_b.from_host(bases)
        self.d_o.from_host(offsets)
        self.kf.push_reads_device(self.d_b.ptr, self.d_o.ptr, n, bases.size)
        self.kf.finalize()
        self.c = capi.Corrector(k=K_CORR)
        self.c.from_kfreq(self.kf, CUTOFF)

    def close(self):
        self.c.close()
        self.d_b.free()
        self.d_o.free()
        self.kf.close()


def handoff():
    from dbg_assembly_amd import capi
    bases, offsets = workload()
    n = len(offsets) - 1
    ch = Chain(capi, bases, offsets)
    res = {}
    try:
        out, rec_h = ch.c.correct(bases, offsets)
        seqs = host_trim(out, offsets, rec_h)
        for engine in ("direct", "partition"):
            rec = ch.c.correct_device(ch.d_b.ptr, offsets)
            assert np.array_equal(rec, rec_h)
            info = ch.c.compact()
            assert info["deleted_reads"] > 0 and info["trimmed_reads"] > 0, info
            with capi.Graph(**graph_args(engine, n)) as g:
                g.push_corrected(ch.c)
                new = result_of(g)
                assert (g.store_room()[1] > 0) == (engine == "partition")
            with capi.Graph(**graph_args(engine, n)) as g:
                g.push_reads(*pack(seqs))
                old = result_of(g)
            same(new, old, engine)
            res[engine] = {"nodes": new[0][2], "kmers": new[0][1], "deleted_reads": info["deleted_reads"], "trimmed_reads": info["trimmed_reads"],
                           "ms_scan": info["ms_scan"], "ms_gather": info["ms_gather"]}
        assert res["direct"]["nodes"] == res["partition"]["nodes"]
    finally:
        ch.close()
    return res


def split_workload():
    """batch A large enough (150 k reads, 15 MB) that the graph's kernels over it are still queued or running when the corrector
    starts on B; B starts on a 16-byte boundary of the resident buffer.  A race that never loses proves nothing: this step
    checks the results of the ordering, it cannot show that the waits are needed"""
    bases, offsets = workload(n_reads=200000, genome=200000)
    n = len(offsets) - 1
    cut = 150000
    assert int(offsets[cut]) % 16 == 0
    return bases, offsets, [(0, cut), (cut, n)]


def host_batches(ch, bases, offsets, parts):
    seqs = []
    for a, b in parts:
        o = offsets[a:b + 1] - offsets[a]
        out, rec = ch.c.correct(bases[int(offsets[a]):int(offsets[b])], o)
        seqs.append(pack(host_trim(out, o, rec)))
    return seqs


def reuse():
    """A compacted and pushed, B corrected, compacted and pushed at once, then finalize; and again with every compact batch pushed twice"""
    from dbg_assembly_amd import capi
    bases, offsets, parts = split_workload()
    n = len(offsets) - 1
    ch = Chain(capi, bases, offsets)
    res = {}
    try:
        seqs = host_batches(ch, bases, offsets, parts)
        for times in (1, 2):
            with capi.Graph(**graph_args("partition", n * times)) as g:
                for a, b in parts:
                    ch.c.correct_device(ch.d_b.ptr + int(offsets[a]), offsets[a:b + 1] - offsets[a])
                    ch.c.compact()
                    for _ in range(times):
                        g.push_corrected(ch.c)
                new = result_of(g)
            with capi.Graph(**graph_args("partition", n * times)) as g:
                for s in seqs:
                    for _ in range(times):
                        g.push_reads(*s)
                old = result_of(g)
            same(new, old, "pushed %d time(s)" % times)
            res["times_%d" % times] = {"reads": new[0][0], "kmers": new[0][1], "nodes": new[0][2]}
        assert res["times_2"]["kmers"] == 2 * res["times_1"]["kmers"] and res["times_2"]["nodes"] == res["times_1"]["nodes"]
    finally:
        ch.close()
    return res


def two_handles():
    """every compact batch goes into TWO handles -- the k = 31 graph first, a KFREQ handle second, so that the event of the second
    push has to cover the first -- and the corrector goes on with the next batch at once"""
    from dbg_assembly_amd import capi
    bases, offsets, parts = split_workload()
    n = len(offsets) - 1
    ch = Chain(capi, bases, offsets)
    try:
        seqs = host_batches(ch, bases, offsets, parts)
        kf_args = dict(k=K_CORR, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000)
        with capi.Graph(**graph_args("partition", n)) as g, capi.Graph(**kf_args) as kf:
            for a, b in parts:
                ch.c.correct_device(ch.d_b.ptr + int(offsets[a]), offsets[a:b + 1] - offsets[a])
                ch.c.compact()
                g.push_corrected(ch.c)
                kf.push_corrected(ch.c)
            new = result_of(g)
            kf.finalize()
            counts_new = kf.kfreq_counts()
        with capi.Graph(**graph_args("partition", n)) as g, capi.Graph(**kf_args) as kf:
            for s in seqs:
                g.push_reads(*s)
                kf.push_reads(*s)
            old = result_of(g)
            kf.finalize()
            counts_old = kf.kfreq_counts()
        same(new, old, "graph")
        assert np.array_equal(counts_new, counts_old) and int(np.count_nonzero(counts_new)) > 100000
    finally:
        ch.close()
    return {"reads": new[0][0], "kmers": new[0][1], "nodes": new[0][2], "kfreq_distinct": int(np.count_nonzero(counts_new))}


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "goldens": goldens, "edges_small": edges_small, "edges_chunks": edges_chunks,
                      "device_input": device_input, "handoff": handoff, "reuse": reuse, "two_handles": two_handles}[sys.argv[1]]()))
