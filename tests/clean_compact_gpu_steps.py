"""GPU steps of tests/test_clean_compact_gpu.py, each run in a child process of its own under a time limit:
    python tests/clean_compact_gpu_steps.py crafted | goldens | edges | device_input | chain | reuse | states
Prints one JSON line of findings; exits non-zero on a mismatch."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_compact_restatement as CC  # noqa: E402
import clean_restatement as CR  # noqa: E402

CASES = os.path.join(ROOT, "tests", "golden", "clean_cases")
PAD = 16   # bytes a plane handed to a _device call must be readable behind its last read


# ---- crafted batches through compact_from ------------------------------------------------------------------------------------------
# a read is (L, start0, keep, trimmed): its record keeps bytes [start0, start0 + keep) when trimmed, the whole read otherwise

def kept(rng, kind, out_lens):
    """trimmed reads with the given OUTPUT lengths: random bytes cut off behind them and, for clean_lowqual, in front of them"""
    rows = []
    for m in out_lens:
        pre = int(rng.integers(0, 20)) if kind == CC.LOWQUAL else 0
        rows.append((int(m) + pre + int(rng.integers(0, 20)), pre, int(m), 1))
    return rows


def whole(lens):
    return [(int(n), 0, int(n), 0) for n in lens]


def emptied(n, L=30):
    """n reads whose record keeps nothing: a block with start 0, a hit with read_start 1"""
    return [(L, 0, 0, 1)] * n


def with_total(rng, kind, total):
    """short reads whose output lengths sum to `total` exactly"""
    lens = []
    while sum(lens) < total:
        lens.append(min(int(rng.integers(1, 101)), total - sum(lens)))
    return kept(rng, kind, lens)


def records(kind, rows):
    """rows -> the records of `kind`.  A block that keeps nothing has start 0; a hit that keeps nothing has read_start 1"""
    if kind == CC.LOWQUAL:
        out = []
        for L, s, m, t in rows:
            if not t:
                out.append((0.5, 1 if L else 0, L, 0))
            else:
                out.append((0.5, s + 1, m, 1) if m else (0.5, 0, 0, 1))
        return CC.blocks_of(out)
    assert all(s == 0 for _, s, _, _ in rows)
    return CC.hits_of([(0, 12, m + 1, min(L, m + 12), 1, 12) if t else CR.NO_HIT for L, _, m, t in rows])


def planes(rng, rows):
    """bases from ACGTNn, qualities from 35 .. 63: no byte occurs in both planes, and none equals a shift of 33 or 64"""
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r[0] for r in rows])
    nb = int(offsets[-1])
    bases = np.frombuffer(b"ACGTNn", dtype=np.uint8)[rng.choice(6, nb, p=[.2, .2, .2, .2, .15, .05])]
    return bases, rng.integers(35, 64, nb, dtype=np.uint8), offsets


def pair_rows(kind):
    """every pair (source start mod 4, destination start mod 4) at output lengths 1, 2, 3, 4, 5 and 17: in front of each target
    read an untrimmed read moves the destination (and the source), an emptied one the source alone -> (rows, target indices)"""
    rows, targets, src, dst = [], [], 0, 0
    pre = 2 if kind == CC.LOWQUAL else 0
    for m in (1, 2, 3, 4, 5, 17):
        for s in range(4):
            for d in range(4):
                x = (d - dst) % 4 + 4
                rows.append((x, 0, x, 0))
                src, dst = src + x, dst + x
                e = (s - src - pre) % 4
                rows.append((e, 0, 0, 1))
                src += e
                targets.append(len(rows))
                rows.append((pre + m + 3, pre, m, 1))
                src, dst = src + pre + m + 3, dst + m
    return rows, targets


def crafted_cases(kind, T):
    rng = np.random.default_rng(20 + kind)
    cases = {}
    cases["n1"] = (kept(rng, kind, [37]), 0)
    cases["all_emptied"] = (emptied(1000), 0)
    rows = kept(rng, kind, rng.integers(1, 101, 4000))
    for i in np.flatnonzero(rng.random(4000) < 0.05):
        rows[i] = (rows[i][0], 0, 0, 1)
    cases["lengths_1_100"] = (rows, 20)
    for name, total in (("total_T", T), ("total_T_plus_1", T + 1), ("total_T_minus_1", T - 1), ("total_15", 15)):
        cases[name] = (with_total(rng, kind, total), 0)
    cases["empty_run_3T_inside_a_tile"] = (with_total(rng, kind, T + 1000) + emptied(3 * T) + with_total(rng, kind, 2 * T), 0)
    cases["empty_run_ends_on_a_tile_boundary"] = (with_total(rng, kind, 2 * T) + emptied(3 * T) + with_total(rng, kind, T + 5), 0)
    cases["empty_run_ends_one_byte_past_a_boundary"] = (with_total(rng, kind, T + 1) + emptied(3 * T) + with_total(rng, kind, 300), 0)
    cases["first_and_last_empty"] = (emptied(1) + with_total(rng, kind, 500) + emptied(1), 0)
    for a in range(16):   # 40 bytes kept, a bytes dropped, then the long read: its source starts at 40 + a, its destination at 40
        cases["long_read_spans_three_tiles_src%d" % a] = (whole([40]) + emptied(1, a) + [(2 * T + 17 + 9, 0, 2 * T + 17, 1)] + kept(rng, kind, [33, 80]), 0)
    cases["source_and_destination_mod_4"] = (pair_rows(kind)[0], 0)
    cases["min_len_boundary"] = (kept(rng, kind, [60, 49, 50, 51, 49, 70, 50, 51]), 50)
    cases["min_len_0_empty_input_reads"] = (whole([0, 30, 0, 0, 45, 0]) + kept(rng, kind, [12]) + whole([0]), 0)
    cases["record_keeps_nothing"] = (whole([50]) + emptied(1, 50) + whole([20]), 0)   # read_start 1 / block start 0
    return cases


def check_crafted(c, g, kind, name, bases, quals, offsets, rec, shift, min_len):
    from dbg_assembly_amd import capi
    want_b, want_q, want_o, want_c = CC.compact(kind, bases, quals, offsets, rec, shift, min_len)
    info = c.compact_from(kind, bases, quals, offsets, rec, shift, min_len)
    got_b, got_q, got_o = c.compact_to_host()
    assert np.array_equal(got_o, want_o), (kind, name)
    assert np.array_equal(got_b, want_b), (kind, name, "bases", int(np.flatnonzero(got_b != want_b)[0]))
    if quals is None:
        assert got_q is None, (kind, name)
    else:
        assert np.array_equal(got_q, want_q), (kind, name, "quals", int(np.flatnonzero(got_q != want_q)[0]))
    assert {f: info[f] for f in CC.COUNTERS} == want_c, (kind, name, info, want_c)
    d_b, d_q, d_o, n, nb = c.compact_device()
    assert (n, nb) == (len(rec), len(want_b)) and d_b % 16 == 0 and d_o % 8 == 0 and (d_q is None) == (quals is None)
    if nb % 16:   # the pad of the last vector of each plane
        for ptr, want in ((d_b, want_b), (d_q, want_q)):
            if ptr:
                tail = np.full(16, 0xAA, dtype=np.uint8)
                assert capi.lib().dbgk_memcpy_d2h(g._h, tail.ctypes.data, ctypes.c_void_p(ptr + nb - nb % 16), 16) == 0
                assert np.array_equal(tail[:nb % 16], want[nb - nb % 16:]) and not tail[nb % 16:].any(), (kind, name)
    return info, want_o


def crafted():
    from dbg_assembly_amd import capi
    T = capi.CLEAN_COMPACT_TILE
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Cleaner() as c:
        for kind, tag in ((CC.LOWQUAL, "lowqual"), (CC.ADAPTER, "adapter")):
            rng = np.random.default_rng(7 + kind)
            clean_reads = {}
            for name, (rows, min_len) in crafted_cases(kind, T).items():
                bases, quals, offsets = planes(rng, rows)
                rec = records(kind, rows)
                info, coff = check_crafted(c, g, kind, name, bases, quals, offsets, rec, 33, min_len)
                res["%s/%s" % (tag, name)] = {"reads": info["reads"], "bases": int(coff[-1])}
                starts = CC.cuts(kind, offsets, rec)[0]
                if name == "all_emptied":
                    assert int(coff[-1]) == 0 and info["ms_gather"] == 0 and info["trimmed_reads"] == 1000
                if name.startswith("long_read_spans_three_tiles"):
                    assert int(coff[2]) == 40 and int(coff[3]) - int(coff[2]) == 2 * T + 17
                    res.setdefault(tag + "/long_read_src_mod16", []).append((int(offsets[2]) + int(starts[2])) % 16)
                if name == "source_and_destination_mod_4":
                    t = pair_rows(kind)[1]
                    seen = {((int(offsets[i]) + int(starts[i])) % 4, int(coff[i]) % 4, int(coff[i + 1] - coff[i])) for i in t}
                    assert seen == {(s, d, m) for s in range(4) for d in range(4) for m in (1, 2, 3, 4, 5, 17)}
                if name == "min_len_boundary":
                    assert np.diff(coff.astype(np.int64)).tolist() == [60, 0, 50, 51, 0, 70, 50, 51] and info["short_reads"] == 2
                if name == "min_len_0_empty_input_reads":
                    clean_reads[kind] = info["clean_reads"]
                    assert info["short_reads"] == 0 and info["reads"] == 8
                if name == "lengths_1_100":   # the same batch without a quality plane
                    check_crafted(c, g, kind, name + ", bases alone", bases, None, offsets, rec, 33, min_len)
            assert sorted(res[tag + "/long_read_src_mod16"]) == list(range(16))
            res[tag + "/clean_reads_of_8_with_5_empty"] = clean_reads[kind]
        assert (res["lowqual/clean_reads_of_8_with_5_empty"], res["adapter/clean_reads_of_8_with_5_empty"]) == (3, 8)
        # N: the first and the last kept byte of the block, one byte before it and one behind it; a lower-case n inside it
        for shift in (33, 64):
            read = bytearray(b"ACGT" * 5)
            for at in (4, 5, 14, 15):
                read[at] = ord("N")
            read[8] = ord("n")
            bases = np.frombuffer(bytes(b"TTTTT" + read + b"GG"), dtype=np.uint8)
            quals = np.arange(35, 35 + bases.size, dtype=np.uint8)
            offsets = np.array([0, 5, 25, 27], dtype=np.uint64)
            rec = CC.blocks_of([(0.0, 1, 5, 0), (1.0, 6, 10, 1), (0.0, 1, 2, 0)])
            check_crafted(c, g, CC.LOWQUAL, "N_shift%d" % shift, bases, quals, offsets, rec, shift, 0)
            _, got_q, coff = c.compact_to_host()
            block = got_q[int(coff[1]):int(coff[2])]
            assert block.size == 10 and np.flatnonzero(block == shift).tolist() == [0, 9] and block[3] == 35 + 5 + 8
            res["lowqual/N_shift%d" % shift] = {"rewritten": int((got_q == shift).sum())}
            # the same bytes under an adapter record: no quality is rewritten
            hits = CC.hits_of([CR.NO_HIT, (0, 12, 16, 20, 1, 5), CR.NO_HIT])
            check_crafted(c, g, CC.ADAPTER, "N_under_a_hit", bases, quals, offsets, hits, shift, 0)
            assert not (c.compact_to_host()[1] == shift).any()
        # records that point outside their read give length 0, their neighbours are untouched
        rng = np.random.default_rng(3)
        bases, quals, offsets = planes(rng, whole([50, 50, 50, 50, 50, 50]))
        rec = CC.blocks_of([(0.0, 1, 50, 0), (1.0, 5, 100, 1), (1.0, 52, 1, 1), (1.0, -3, 10, 1), (1.0, 10, -1, 1), (1.0, 41, 10, 1)])
        info, coff = check_crafted(c, g, CC.LOWQUAL, "outside", bases, quals, offsets, rec, 33, 0)
        assert np.diff(coff.astype(np.int64)).tolist() == [50, 0, 0, 0, 0, 10] and info["trimmed_reads"] == 5
        hits = CC.hits_of([CR.NO_HIT, (0, 12, 60, 70, 1, 11), (0, 12, 52, 60, 1, 9), (0, 12, -4, 8, 1, 12), (0, 12, 0, 5, 1, 5), (0, 12, 51, 51, 1, 1)])
        info, coff = check_crafted(c, g, CC.ADAPTER, "outside", bases, quals, offsets, hits, 33, 0)
        assert np.diff(coff.astype(np.int64)).tolist() == [50, 0, 0, 0, 0, 50] and info["trimmed_reads"] == 5
        res["outside"] = {"lowqual": 4, "adapter": 4}
    return res


# ---- goldens and edge scenarios: the batch calls, then compact() -------------------------------------------------------------------
class Upload:
    """two planes in device memory, PAD readable bytes behind the last read"""

    def __init__(self, g, bases, quals):
        self.size = int(np.asarray(bases).size)
        self.b, self.q = g.malloc(self.size + PAD), g.malloc(self.size + PAD)
        self.fill = np.full(self.size + PAD, 0x5A, dtype=np.uint8)
        for buf, plane in ((self.b, bases), (self.q, quals)):
            buf.from_host(self.fill)
            if self.size:
                buf.from_host(np.ascontiguousarray(plane, dtype=np.uint8))

    def unchanged(self, bases, quals):
        for buf, plane in ((self.b, bases), (self.q, quals)):
            got = buf.to_host(np.uint8, self.size + PAD)
            if not (np.array_equal(got[:self.size], plane) and np.array_equal(got[self.size:], self.fill[self.size:])):
                return False
        return True

    def free(self):
        self.b.free()
        self.q.free()


def run_batch(c, g, kind, reads, quals, opts):
    """host input, then device input with both planes: the records agree, and so do the compact batches
    -> (lines 2, lines 4, counters, records).  dbgk_clean_adapter takes no qualities, so line 4 of an adapter batch comes from the
    device-input call alone"""
    bases, offsets = CC.pack(reads)
    qplane, _ = CC.pack(quals)
    up = Upload(g, bases, qplane)
    try:
        if kind == CC.ADAPTER:
            rec_h = c.adapter(bases, offsets)
            info_h = c.compact(opts["-r"])
            b_h, q_h, o_h = c.compact_to_host()
            assert q_h is None
            rec_d = c.adapter_device(up.b.ptr, up.q.ptr, offsets)
        else:
            rec_h = c.lowqual(bases, qplane, offsets, opts["-e"], opts["-q"])
            info_h = c.compact(opts["-r"])
            b_h, q_h, o_h = c.compact_to_host()
            rec_d = c.lowqual_device(up.b.ptr, up.q.ptr, offsets, opts["-e"], opts["-q"])
        info_d = c.compact(opts["-r"])
        b_d, q_d, o_d = c.compact_to_host()
        assert up.unchanged(bases, qplane), "the caller's planes were written"
    finally:
        up.free()
    assert rec_d.tobytes() == rec_h.tobytes()
    assert np.array_equal(b_d, b_h) and np.array_equal(o_d, o_h) and (q_h is None or np.array_equal(q_d, q_h))
    assert all(info_d[f] == info_h[f] for f in CC.COUNTERS), (info_d, info_h)
    lines4 = CC.as_lines(q_d, o_d) if q_d is not None else [b""] * (len(o_d) - 1)   # (no reads: no plane)
    return CC.as_lines(b_d, o_d), lines4, {f: info_d[f] for f in CC.COUNTERS}, rec_d


def goldens():
    from dbg_assembly_amd import capi
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Cleaner() as c:
        for case in CR.golden_cases(CASES):
            b = CC.golden_batch(CASES, case)
            if b["kind"] == CC.ADAPTER:
                c.set_adapters([s for _, s in CR.case_adapters(CASES, case)], b["opts"]["-s"])
            lines2, lines4, cnt, _ = run_batch(c, g, b["kind"], b["reads"], b["quals"], b["opts"])
            assert lines2 == b["lines2"], case["name"]
            assert lines4 == b["lines4"], case["name"]
            assert cnt == b["stat"], (case["name"], cnt, b["stat"])
            res[case["name"]] = cnt
    return res


def edges():
    """every pinned scenario of clean_edge_cases.py with -r 0, as its golden was written: compact() against what Cleaner.trim_* makes
    of the same records"""
    from dbg_assembly_amd import capi
    import clean_edge_cases as E
    from test_clean_compact_cpu import edge_batch
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Cleaner() as c:
        for s in E.scenarios():
            if not E.pinned(s):
                continue
            kind, reads, quals, shift = edge_batch(s)
            recs = [("@%d" % i, E.text(r), E.text(q)) for i, (r, q) in enumerate(zip(reads, quals))]
            if kind == CC.ADAPTER:
                c.set_adapters([a for _, a in s.adapters], s.cutoff)
                out, _ = c.trim_adapter(recs, [i for i, _ in s.adapters], 0)
                opts = {"-r": 0}
            else:
                out, _ = c.trim_lowqual(recs, s.cutoff, s.shift, 0)
                opts = {"-r": 0, "-e": s.cutoff, "-q": s.shift}
            lines2, lines4, cnt, rec = run_batch(c, g, kind, reads, quals, opts)
            assert lines2 == [r[1].encode("latin-1") for r in out], s.name
            assert lines4 == [r[2].encode("latin-1") for r in out], s.name
            assert cnt == CC.trim_rule(kind, reads, quals, rec.tolist(), shift, 0)[2], s.name
            res[s.name] = {"reads": cnt["reads"], "trimmed_reads": cnt["trimmed_reads"], "clean_bases": cnt["clean_bases"]}
    return res


# ---- device input against host input ---------------------------------------------------------------------------------------------------
def device_input():
    """a few thousand reads of mixed lengths (some beyond the LDS slice of the adapter kernel, some empty): the _device calls on planes
    the test uploaded give the records and the compact batch of the host-input calls and leave the planes as they were (run_batch),
    and both equal the restatement"""
    from dbg_assembly_amd import capi
    from clean_gpu_steps import synthetic_job
    reads, adapters = synthetic_job(3000)
    rng = np.random.default_rng(9)
    quals = [(33 + rng.choice([40, 40, 41, 37, 30, 20, 12, 2], len(r), p=[.4, .2, .1, .1, .08, .06, .04, .02])).astype(np.uint8).tobytes()
             for r in reads]
    bases, offsets = CC.pack(reads)
    qplane, _ = CC.pack(quals)
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Cleaner() as c:
        c.set_adapters([s for _, s in adapters], 10)
        for kind, tag, opts in ((CC.ADAPTER, "adapter", {"-r": 10}), (CC.LOWQUAL, "lowqual", {"-r": 10, "-e": 0.01, "-q": 33})):
            lines2, lines4, cnt, rec = run_batch(c, g, kind, reads, quals, opts)
            want_b, want_q, want_o, want_c = CC.compact(kind, bases, qplane, offsets, rec, 33, 10)
            assert lines2 == CC.as_lines(want_b, want_o) and lines4 == CC.as_lines(want_q, want_o) and cnt == want_c, tag
            assert cnt["trimmed_reads"] > 0 and cnt["short_reads"] > 0 and cnt["clean_reads"] > 0, cnt
            res[tag] = cnt
    return res


# ---- one upload from raw reads to the table and the graph ----------------------------------------------------------------------------
READ_LEN, MIN_LEN, N_CHAIN, K_FREQ, K_GRAPH, CUTOFF = 150, 75, 4000, 17, 31, 2
ADAPTER_SEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"


def workload(n_reads=N_CHAIN, genome=20000, seed=5):
    """150-bp reads drawn from a random genome with 0.5 % substitutions (30-fold coverage: work for the corrector), Q40 throughout.
    About one read in six ends in the adapter and random bases behind it (from a base before or behind MIN_LEN), about one in six
    has a low-quality tail (shorter or longer than half the read), one in a hundred holds an N -> (reads, quals) as lists of bytes"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = letters[rng.integers(0, 4, genome)]
    ad = np.frombuffer(ADAPTER_SEQ.encode(), dtype=np.uint8)
    reads, quals = [], []
    for i in range(n_reads):
        p = int(rng.integers(0, genome - READ_LEN))
        s = g[p:p + READ_LEN].copy()
        err = np.flatnonzero(rng.random(READ_LEN) < 0.005)
        s[err] = letters[rng.integers(0, 4, len(err))]
        q = np.full(READ_LEN, 33 + 40, dtype=np.uint8)
        if i % 6 == 1:
            cut = int(rng.integers(10, READ_LEN - len(ad)))
            s[cut:cut + len(ad)] = ad
            s[cut + len(ad):] = letters[rng.integers(0, 4, READ_LEN - cut - len(ad))]
        if i % 6 == 4:
            q[READ_LEN - int(rng.integers(10, 140)):] = 33 + 2
        if i % 100 == 7:
            s[int(rng.integers(0, READ_LEN))] = ord("N")
        reads.append(s.tobytes())
        quals.append(q.tobytes())
    return reads, quals


def host_route(capi, reads, quals):
    """today's route: trim_lowqual, then trim_adapter on what it wrote -> (reads, quals) as lists of bytes"""
    recs = [("@%d" % i, r.decode("latin-1"), q.decode("latin-1")) for i, (r, q) in enumerate(zip(reads, quals))]
    with capi.Cleaner() as c:
        c.set_adapters([ADAPTER_SEQ], 12)
        out, _ = c.trim_lowqual(recs, 0.001, 33, MIN_LEN)
        out, _ = c.trim_adapter(out, ["adapter"], MIN_LEN)
    return [r[1].encode("latin-1") for r in out], [r[2].encode("latin-1") for r in out]


class Stages:
    """the two cleaning stages on two handles: lowqual on the caller's planes, adapter on the first handle's compact planes"""

    def __init__(self, capi):
        self.low, self.ad = capi.Cleaner(), capi.Cleaner()
        self.ad.set_adapters([ADAPTER_SEQ], 12)

    def run(self, d_bases, d_quals, offsets):
        self.low.lowqual_device(d_bases, d_quals, offsets, 0.001, 33)
        info_low = self.low.compact(MIN_LEN)
        b, q, _, n, _ = self.low.compact_device()
        off_low = self.low.compact_to_host()[2]
        assert n == len(offsets) - 1
        self.ad.adapter_device(b, q, off_low)
        return info_low, off_low, self.ad.compact(MIN_LEN)

    def close(self):
        self.low.close()
        self.ad.close()


def graph_args(capi, engine, n_reads):
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


def tables_equal(kf_a, kf_b):
    """two finalized KFREQ handles hold the same counters.  At k = 17 a table is 16 GiB: the two are compared where they lie, a GiB
    at a time, and one slice is also compared as kfreq_counts exports it -> the number of non-zero counters"""
    import torch
    from dbg_assembly_amd.multigpu import wrap_device_memory
    (pa, na), (pb, nb) = kf_a.kfreq_device_counts(), kf_b.kfreq_device_counts()
    assert na == nb == 4 ** kf_a.k
    a, b = wrap_device_memory(pa, na, "cuda:0"), wrap_device_memory(pb, nb, "cuda:0")
    distinct = 0
    for at in range(0, na, 1 << 30):
        assert bool(torch.equal(a[at:at + (1 << 30)], b[at:at + (1 << 30)])), at
        distinct += int(torch.count_nonzero(a[at:at + (1 << 30)]))
    head_a, head_b = kf_a.kfreq_counts(0, 1 << 26), kf_b.kfreq_counts(0, 1 << 26)
    assert np.array_equal(head_a, head_b) and int(np.count_nonzero(head_a)) == int(torch.count_nonzero(a[:1 << 26]))
    return distinct


def chain():
    from dbg_assembly_amd import capi
    import corr_compact_restatement as CO
    reads, quals = workload()
    n = len(reads)
    bases, offsets = CC.pack(reads)
    qplane, _ = CC.pack(quals)
    want_reads, want_quals = host_route(capi, reads, quals)
    want_bases, want_off = CC.pack(want_reads)
    res = {}
    kf_args = dict(k=K_FREQ, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000)
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g0:
        up, st = Upload(g0, bases, qplane), Stages(capi)   # the one upload
        try:
            info_low, off_low, info_ad = st.run(up.b.ptr, up.q.ptr, offsets)
            got_b, got_q, got_o = st.ad.compact_to_host()
            len_low, len_ad = np.diff(off_low.astype(np.int64)), np.diff(got_o.astype(np.int64))
            res["emptied_by_lowqual"], res["emptied_by_adapter"] = int((len_low == 0).sum()), int(((len_low > 0) & (len_ad == 0)).sum())
            res["kept"], res["cut_and_kept"] = int((len_ad > 0).sum()), int(((len_ad > 0) & (len_ad < READ_LEN)).sum())
            assert min(res.values()) > 0, res
            assert CC.as_lines(got_b, got_o) == want_reads and CC.as_lines(got_q, got_o) == want_quals
            assert up.unchanged(bases, qplane)
            with capi.Graph(**kf_args) as kf_new, capi.Graph(**kf_args) as kf_old:
                kf_new.push_cleaned(st.ad)
                kf_new.finalize()
                kf_old.push_reads(want_bases, want_off)
                kf_old.finalize()
                res["kfreq_distinct"] = tables_equal(kf_new, kf_old)
                assert res["kfreq_distinct"] > 10000
                with capi.Corrector(k=K_FREQ) as c:
                    c.from_kfreq(kf_new, CUTOFF)
                    out_h, rec_h = c.correct(want_bases, want_off)
                    c.compact()
                    cb_h, co_h = c.compact_to_host()
                    d_b, _, _, _, _ = st.ad.compact_device()
                    rec_d = c.correct_device(d_b, got_o)
                    c.compact()
                    cb_d, co_d = c.compact_to_host()
                assert np.array_equal(rec_d, rec_h), "the corrector's records differ"
                assert np.array_equal(cb_d, cb_h) and np.array_equal(co_d, co_h), "the corrected bytes differ"
                assert np.array_equal(cb_d, CO.compact(out_h, want_off, rec_h)[0])
                res["corrected_bases"] = int(rec_h["one_base"].sum() + rec_h["tree"].sum())
                assert res["corrected_bases"] > 0 and int(rec_h["deleted"].sum()) > 0, res
            for engine in ("direct", "partition"):
                with capi.Graph(**graph_args(capi, engine, n)) as g:
                    g.push_cleaned(st.ad)
                    new = result_of(g)
                    assert (g.store_room()[1] > 0) == (engine == "partition")
                with capi.Graph(**graph_args(capi, engine, n)) as g:
                    g.push_reads(want_bases, want_off)
                    old = result_of(g)
                same(new, old, engine)
                res[engine] = {"nodes": new[0][2], "kmers": new[0][1]}
            assert res["direct"]["nodes"] == res["partition"]["nodes"] > 1000
            res["ms"] = {"lowqual": [info_low["ms_scan"], info_low["ms_gather"]], "adapter": [info_ad["ms_scan"], info_ad["ms_gather"]]}
        finally:
            st.close()
            up.free()
    return res


def reuse():
    """two batches of the resident reads: each is cleaned, compacted and pushed into TWO handles -- the k = 31 graph first, a KFREQ
    handle second, so that the event of the second push has to cover the first -- and both cleaners go on with the next batch at
    once, before either handle is synced.  A race that never loses proves nothing: this step checks the results of the ordering,
    it cannot show that the waits are needed"""
    from dbg_assembly_amd import capi
    reads, quals = workload()
    n, cut = len(reads), 2400
    bases, offsets = CC.pack(reads)
    qplane, _ = CC.pack(quals)
    assert int(offsets[cut]) % 16 == 0
    want_reads, _ = host_route(capi, reads, quals)
    parts = [(0, cut), (cut, n)]
    kf_args = dict(k=13, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000)
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g0:
        up, st = Upload(g0, bases, qplane), Stages(capi)
        try:
            with capi.Graph(**graph_args(capi, "partition", n)) as g, capi.Graph(**kf_args) as kf:
                for a, b in parts:
                    st.run(up.b.ptr + int(offsets[a]), up.q.ptr + int(offsets[a]), offsets[a:b + 1] - offsets[a])
                    g.push_cleaned(st.ad)
                    kf.push_cleaned(st.ad)
                new = result_of(g)
                kf.finalize()
                counts_new = kf.kfreq_counts()
            with capi.Graph(**graph_args(capi, "partition", n)) as g, capi.Graph(**kf_args) as kf:
                for a, b in parts:
                    batch = CC.pack(want_reads[a:b])
                    g.push_reads(*batch)
                    kf.push_reads(*batch)
                old = result_of(g)
                kf.finalize()
                counts_old = kf.kfreq_counts()
        finally:
            st.close()
            up.free()
    same(new, old, "graph")
    assert np.array_equal(counts_new, counts_old) and int(np.count_nonzero(counts_new)) > 10000
    return {"reads": new[0][0], "kmers": new[0][1], "nodes": new[0][2], "kfreq_distinct": int(np.count_nonzero(counts_new))}


# ---- the error returns -------------------------------------------------------------------------------------------------------------------
def status_of(call):
    from dbg_assembly_amd import capi
    try:
        call()
    except capi.DbgkError as e:
        return e.status
    return capi.OK


def states():
    from dbg_assembly_amd import capi
    reads, quals = workload(200)
    bases, offsets = CC.pack(reads)
    qplane, _ = CC.pack(quals)
    res = {}
    with capi.Graph(k=31, table_slots=capi.find_next_prime_ref(100000), engine=capi.ENGINE_DIRECT) as g, capi.Cleaner() as c:
        res["compact_before_any_batch"] = status_of(lambda: c.compact(MIN_LEN))
        res["device_before_any_compact"] = status_of(c.compact_device)
        res["push_before_any_compact"] = status_of(lambda: g.push_cleaned(c))
        c.set_adapters([ADAPTER_SEQ], 12)
        up = Upload(g, bases, qplane)
        try:
            hits = c.adapter_device(up.b.ptr, None, offsets)
            assert np.array_equal(hits, c.adapter(bases, offsets))
            c.adapter_device(up.b.ptr, None, offsets)
            info = c.compact(MIN_LEN)
            got_b, got_q, got_o = c.compact_to_host()
            d_b, d_q, _, n, nb = c.compact_device()
            assert got_q is None and d_q is None and n == len(reads) and nb == got_b.size == info["clean_bases"] > 0
            assert np.array_equal(got_b, CC.compact(CC.ADAPTER, bases, None, offsets, hits, 33, MIN_LEN)[0])
            q = np.zeros(max(nb, 1), dtype=np.uint8)
            res["quality_plane_of_a_batch_without_one"] = capi.lib().dbgk_clean_compact_results(c._h, None, q.ctypes.data, None)
            res["results_with_no_pointer"] = capi.lib().dbgk_clean_compact_results(c._h, None, None, None)
            c.lowqual_device(up.b.ptr, up.q.ptr, offsets)
            c.compact(MIN_LEN)
            own_b, own_q, _, _, _ = c.compact_device()
            own_off = c.compact_to_host()[2]
            res["own_bases_as_adapter_input"] = status_of(lambda: c.adapter_device(own_b, None, own_off))
            res["own_quals_as_adapter_quals"] = status_of(lambda: c.adapter_device(up.b.ptr, own_q, offsets))
            res["own_planes_as_lowqual_input"] = status_of(lambda: c.lowqual_device(own_b, own_q, own_off))
            res["misaligned_plane"] = status_of(lambda: c.adapter_device(up.b.ptr + 4, None, offsets[:2]))
            res["negative_min_len"] = status_of(lambda: c.compact(-1))
            res["compact_after_the_refusals"] = status_of(lambda: c.compact(MIN_LEN))   # the batch is still the lowqual batch
            g.push_cleaned(c)
            g.finalize()
            res["push_into_a_finalized_handle"] = status_of(lambda: g.push_cleaned(c))
        finally:
            up.free()
    return res


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "goldens": goldens, "edges": edges, "device_input": device_input, "chain": chain, "reuse": reuse,
                      "states": states}[sys.argv[1]]()))
