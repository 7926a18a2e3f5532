"""GPU steps of tests/test_pair_gpu.py, each run in a child process of its own under a time limit:
    python tests/pair_gpu_steps.py crafted | many | subrange | goldens | cli | graph | mapper | reuse | states
Prints one JSON line of findings; exits non-zero on a mismatch."""
import ctypes
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_restatement as PR  # noqa: E402

EXE = os.path.join(ROOT, "dbg_assembly_amd", "bin", "correct_error_reads")
BOTH, ONLY1, ONLY2, NEITHER = 0, 1, 2, 3
SENTINEL = 0xEE   # no base and no quality below has this value


# ---- crafted batches ---------------------------------------------------------------------------------------------------------------------
def batch(rng, classes, len1, len2):
    """pairs of the given classes: mate m of pair i has len<m>[i] bytes unless its class empties it -> ((b1, o1, q1), (b2, o2, q2)).
    Bases are drawn from ACGTN; a quality byte is a function of (mate, read, position), so a swapped plane or read shows"""
    classes = np.asarray(classes, dtype=np.int64)
    out = []
    for mate, lens in enumerate((len1, len2)):
        lens = np.where((classes == BOTH) | (classes == (ONLY1 if mate == 0 else ONLY2)), np.asarray(lens, dtype=np.int64), 0)
        assert ((lens > 0) == ((classes == BOTH) | (classes == (ONLY1 if mate == 0 else ONLY2)))).all()
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        nb = int(off[-1])
        bases = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, nb)]
        read = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
        pos = np.arange(nb, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), lens)
        quals = (33 + (mate * 47 + read * 13 + pos * 5) % 97).astype(np.uint8)
        out.append((bases, off, quals))
    return tuple(out)


def with_total(rng, total):
    """an even number of read lengths that sum to `total` exactly"""
    lens = []
    while sum(lens) < total:
        lens.append(min(int(rng.integers(1, 101)), total - sum(lens)))
    if len(lens) % 2:
        i = int(np.argmax(lens))
        if lens[i] >= 2:
            lens[i:i + 1] = [lens[i] // 2, lens[i] - lens[i] // 2]
        else:
            lens[:2] = [2]
    assert sum(lens) == total and len(lens) % 2 == 0 and min(lens) > 0
    return lens


def kept_pairs(rng, total):
    """kept pairs whose PAIR bytes sum to `total` -> (classes, len1, len2)"""
    lens = with_total(rng, total)
    return [BOTH] * (len(lens) // 2), lens[0::2], lens[1::2]


def singles(rng, total):
    """pairs with one mate left, alternating between the mates, whose SINGLE bytes sum to `total`"""
    lens = with_total(rng, total)
    return [ONLY1 if i % 2 == 0 else ONLY2 for i in range(len(lens))], lens, lens


def dropped(n, cls=NEITHER):
    return [cls] * n, [30] * n, [30] * n


def join(*parts):
    return tuple(sum((list(p[i]) for p in parts), []) for i in range(3))


def cycling(n):
    return [i % 4 for i in range(n)], [1 + i % 100 for i in range(n)], [1 + (7 * i + 3) % 100 for i in range(n)]


def crafted_cases(T):
    rng = np.random.default_rng(11)
    cases = {"n0": ([], [], [])}
    for cls, tag in ((BOTH, "both"), (ONLY1, "only1"), (ONLY2, "only2"), (NEITHER, "neither")):
        cases["n1_" + tag] = ([cls], [37], [41])
    cases["all_pairs_kept"] = kept_pairs(rng, 30000)
    cases["none_kept"] = dropped(1000)
    cases["all_single_from_mate1"] = ([ONLY1] * 700, list(rng.integers(1, 101, 700)), [9] * 700)
    cases["all_single_from_mate2"] = ([ONLY2] * 700, [9] * 700, list(rng.integers(1, 101, 700)))
    for n in (63, 64, 65, 255, 256, 257):
        cases["classes_cycle_n%d" % n] = cycling(n)
    n = 4000
    cases["lengths_1_100"] = (list(rng.choice(4, n, p=[.55, .2, .2, .05])), [1 + i % 100 for i in range(n)], [1 + (i * 37 + 11) % 100 for i in range(n)])
    for total, tag in ((15, "15"), (16, "16"), (17, "17"), (T - 1, "T_minus_1"), (T, "T"), (T + 1, "T_plus_1")):
        cases["pair_total_" + tag] = join(dropped(3), kept_pairs(rng, total), dropped(2, ONLY1))
        cases["single_total_" + tag] = join(dropped(3, BOTH), singles(rng, total), dropped(2))
    cases["long_read_is_mate2_of_a_kept_pair"] = join(([BOTH], [40], [30]), ([ONLY2], [9], [5]), ([BOTH], [10], [2 * T + 5]), kept_pairs(rng, 300))
    cases["dropped_run_3T_inside_a_tile"] = join(kept_pairs(rng, T + 1000), dropped(3 * T), kept_pairs(rng, 2 * T))
    cases["dropped_run_3T_at_a_tile_boundary"] = join(kept_pairs(rng, 2 * T), dropped(3 * T), kept_pairs(rng, T + 6))
    cases["single_run_3T_between_kept_pairs"] = join(kept_pairs(rng, T + 1000), dropped(3 * T, ONLY2), kept_pairs(rng, 500))
    cases["first_and_last_dropped"] = join(dropped(1), kept_pairs(rng, 500), singles(rng, 90), dropped(1))
    cases["first_and_last_kept"] = join(kept_pairs(rng, 60), dropped(5), singles(rng, 90), kept_pairs(rng, 70))
    return cases


def fetch(g, ptr, nbytes):
    from dbg_assembly_amd import capi
    out = np.full(max(nbytes, 1), 0xAA, dtype=np.uint8)
    if nbytes:
        assert capi.lib().dbgk_memcpy_d2h(g._h, out.ctypes.data, ctypes.c_void_p(ptr), nbytes) == 0
    return out[:nbytes]


def check(p, g, info, want, name, with_qual):
    """both outputs of the last split against the restatement: whole 16-byte vectors of every plane (the pad included), offsets, source
    ids, counters, the longest read"""
    out, counters, max_len = want
    assert {f: info[f] for f in PR.COUNTERS} == counters, (name, info, counters)
    assert info["max_len"] == max_len, (name, info["max_len"], max_len)
    for which in (PR.PAIRED, PR.SINGLE):
        want_b, want_q, want_o, want_ids = out[which]
        got_b, got_q, got_o, got_ids = p.results(which)
        assert np.array_equal(got_o, want_o), (name, which, "offsets")
        assert np.array_equal(got_ids, want_ids), (name, which, "ids")
        d_b, d_q, d_o, n, nb = p.device(which)
        assert (n, nb) == (len(want_ids), int(want_o[-1])) and d_b % 16 == 0 and d_o % 8 == 0 and (d_q is not None) == with_qual, (name, which)
        for ptr, got, plane, what in ((d_b, got_b, want_b, "bases"), (d_q, got_q, want_q, "quals")):
            if plane is None:
                assert got is None
                continue
            vec = fetch(g, ptr, plane.size)
            assert np.array_equal(vec, plane), (name, which, what, int(np.flatnonzero(vec != plane)[0]))
            assert np.array_equal(got, plane[:nb]), (name, which, what)
    return counters


def run_cases(cases, res):
    from dbg_assembly_amd import capi
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Pairer() as p:
        for name, (classes, len1, len2) in cases.items():
            rng = np.random.default_rng(len(name) + len(classes))
            (b1, o1, q1), (b2, o2, q2) = batch(rng, classes, len1, len2)
            for with_qual in (False, True):
                qa, qb = (q1, q2) if with_qual else (None, None)
                want = PR.split(b1, o1, b2, o2, qa, qb)
                info = p.split(b1, o1, b2, o2, qa, qb)
                assert info["n_pairs_in"] == len(classes)
                res[name] = check(p, g, info, want, name, with_qual)
                if not (info["pair_bases"] or info["single_bases"]):
                    assert info["ms_gather"] == 0
            yield name, want, (o1, o2)


def crafted():
    from dbg_assembly_amd import capi
    T = capi.CORR_COMPACT_TILE
    res = {}
    for name, (out, counters, _), (o1, o2) in run_cases(crafted_cases(T), res):
        if name.startswith("pair_total_") or name.startswith("single_total_"):
            key, total = name.split("_total_")
            total = {"15": 15, "16": 16, "17": 17, "T_minus_1": T - 1, "T": T, "T_plus_1": T + 1}[total]
            assert counters[key + "_bases"] == total, (name, counters)
        if name == "long_read_is_mate2_of_a_kept_pair":
            off, ids = out[PR.PAIRED][2], out[PR.PAIRED][3]
            r = int(np.flatnonzero(np.diff(off.astype(np.int64)) == 2 * T + 5)[0])
            assert ids[r] % 2 == 1 and int(off[r]) // T + 2 == (int(off[r + 1]) - 1) // T
        if name == "lengths_1_100":   # every residue of source start and destination start, for both planes, in both outputs
            src = (o1[:-1].astype(np.int64), o2[:-1].astype(np.int64))
            for which in (PR.PAIRED, PR.SINGLE):
                off, ids = out[which][2][:-1].astype(np.int64), out[which][3].astype(np.int64)
                for mate in (0, 1):
                    pick = ids % 2 == mate
                    s, d = src[mate][ids[pick] >> 1], off[pick]
                    assert set((s % 16).tolist()) == set(range(16)) and set((d % 16).tolist()) == set(range(16)), (which, mate)
                    assert {(int(a), int(b)) for a, b in zip(s % 4, d % 4)} == {(a, b) for a in range(4) for b in range(4)}, (which, mate)
            res["lengths_1_100_residues"] = "all"
    return res


def many():
    """70 000 pairs in a fixed-seed class pattern: the rank crosses many workgroups"""
    rng = np.random.default_rng(70000)
    n = 70000
    cases = {"n70000": (list(rng.choice(4, n, p=[.6, .15, .15, .1])), list(rng.integers(1, 61, n)), list(rng.integers(1, 61, n)))}
    res = {}
    for _ in run_cases(cases, res):
        pass
    return res


def subrange():
    """device input whose batches are sub-ranges of larger buffers: both start in the middle of a dword, the second far inside its
    buffer.  Everything outside [off[0], off[n]) holds a sentinel that no read holds: the outputs equal the restatement and hold no
    sentinel, so nothing outside the range is reflected in them"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(5)
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Pairer() as p:
        for front1, front2, tail in ((5, 16 * 37 + 3, 64), (1, 2, 16), (3, 4096 + 7, 1)):
            n = 900
            (b1, o1, q1), (b2, o2, q2) = batch(rng, rng.choice(4, n, p=[.5, .2, .2, .1]), rng.integers(1, 90, n), rng.integers(1, 90, n))
            bufs, planes, offs = [], [], []
            for front, b, q, o in ((front1, b1, q1, o1), (front2, b2, q2, o2)):
                size = front + b.size + tail
                size += -size % 16
                for plane in (b, q):
                    host = np.full(size, SENTINEL, dtype=np.uint8)
                    host[front:front + plane.size] = plane
                    d = g.malloc(size)
                    d.from_host(host)
                    bufs.append(d)
                    planes.append(host)
                off = o + np.uint64(front)
                d = g.malloc(off.nbytes)
                d.from_host(off)
                bufs.append(d)
                offs.append(off)
            try:
                for with_qual in (False, True):
                    want = PR.split(planes[0], offs[0], planes[2], offs[1], planes[1] if with_qual else None, planes[3] if with_qual else None)
                    info = p.split_device(bufs[0].ptr, bufs[2].ptr, bufs[3].ptr, bufs[5].ptr, n, bufs[1].ptr if with_qual else None,
                                          bufs[4].ptr if with_qual else None)
                    check(p, g, info, want, "subrange", with_qual)
                    for which in (PR.PAIRED, PR.SINGLE):
                        for plane in want[0][which][:2]:
                            assert plane is None or not (plane == SENTINEL).any()
                for d, host in zip((bufs[0], bufs[1], bufs[3], bufs[4]), planes):
                    assert np.array_equal(d.to_host(np.uint8, host.size), host), "an input plane was written"
            finally:
                for d in bufs:
                    d.free()
            res["front_%d_%d" % (front1, front2)] = {f: info[f] for f in PR.COUNTERS}
    return res


# ---- the reference's files -----------------------------------------------------------------------------------------------------------------
def seq_lines(text):
    return text.split(b"\n")[1::2]


def golden(name):
    return (gzip.open(os.path.join(PR.GOLDEN, name + ".pair.fa.gz"), "rb").read(), gzip.open(os.path.join(PR.GOLDEN, name + ".single.fa.gz"), "rb").read(),
            open(os.path.join(PR.GOLDEN, name + ".pair.single.stat"), "rb").read())


def goldens():
    """both mate files corrected and compacted by two handles, the two compact batches split where they lie"""
    from dbg_assembly_amd import capi
    import correct_restatement as CR
    from test_correct_cpu import params_of
    meta = {c["name"]: c for c in json.load(open(os.path.join(PR.CORRECT, "cases.json")))}
    recs = CR.read_records(os.path.join(PR.CORRECT, "reads.fq.gz"), 1)
    mates = [PR.pack([s.encode() if isinstance(s, str) else s for _, s in r]) for r in (recs, PR.rotate(recs))]
    res = {}
    for name, (case, _, _) in PR.CASES.items():
        P = params_of(meta[case])
        kw = dict(k=P.k, m=P.m, c=P.c, x=P.x, n=P.n, r=P.r)
        with capi.Corrector(**kw) as c1, capi.Corrector(**kw) as c2, capi.Pairer() as p:
            dev = []
            for c, (bases, offsets) in zip((c1, c2), mates):
                c.load_file(os.path.join(PR.CORRECT, "table.cz"))
                c.correct(bases, offsets)
                c.compact()
                dev.append(c.compact_device())
            assert dev[0][2] == dev[1][2] == len(recs)
            info = p.split_device(dev[0][0], dev[0][1], dev[1][0], dev[1][1], len(recs))
            pair, single, stat = golden(name)
            for which, text in ((PR.PAIRED, pair), (PR.SINGLE, single)):
                bases, quals, off, _ = p.results(which)
                assert quals is None and PR.as_lines(bases, off) == seq_lines(text), (name, which)
            assert PR.stat_text(info).encode() == stat, (name, info)
            res[name] = {f: info[f] for f in PR.COUNTERS}
    return res


def rotated_fq(src, dst):
    lines = gzip.open(src, "rb").read().split(b"\n")
    recs = [lines[i:i + 4] for i in range(0, len(lines) - 1, 4)]
    with open(dst, "wb") as f:
        f.write(b"".join(b"\n".join(r) + b"\n" for r in recs[1:] + recs[:1]))


def cli():
    """bin/correct_error_reads -j 1 as a program on a temporary copy of the reads: the three merged files of the pair equal the
    reference's after decompression, the per-file outputs are what they are without -j 1; two files with different record counts
    are refused at merge time"""
    meta = {c["name"]: c for c in json.load(open(os.path.join(PR.CORRECT, "cases.json")))}
    res = {}
    for name, (case, _, _) in PR.CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            f1, f2 = os.path.join(tmp, "reads_1.fq.gz"), os.path.join(tmp, "reads_2.fq")
            shutil.copy(os.path.join(PR.CORRECT, "reads.fq.gz"), f1)
            rotated_fq(f1, f2)
            with open(os.path.join(tmp, "reads.lib"), "w") as f:
                f.write("%s\n%s\n" % (f1, f2))
            r = subprocess.run([EXE] + meta[case]["args"] + ["-j", "1", os.path.join(PR.CORRECT, "table.cz"), os.path.join(tmp, "reads.lib")],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr[-2000:]
            assert "Merge all the paired reads files completed" in r.stderr
            pair, single, stat = golden(name)
            assert gzip.open(f1 + ".correct.fa.gz.pair.fa.gz", "rb").read() == pair, name
            assert gzip.open(f1 + ".correct.fa.gz.single.fa.gz", "rb").read() == single, name
            assert open(f1 + ".correct.fa.gz.pair.single.stat", "rb").read() == stat, name
            per_file = gzip.open(os.path.join(PR.CORRECT, case + ".correct.fa.gz"), "rb").read()
            assert gzip.open(f1 + ".correct.fa.gz", "rb").read() == per_file, name
            assert open(f1 + ".correct.stat", "rb").read() == open(os.path.join(PR.CORRECT, case + ".correct.stat"), "rb").read(), name
            rec = per_file.split(b"\n")[:-1]
            assert gzip.open(f2 + ".correct.fa.gz", "rb").read() == b"".join(x + b"\n" for x in rec[2:] + rec[:2]), name
            assert sorted(os.listdir(tmp)) == sorted(["reads.lib", "reads_1.fq.gz", "reads_2.fq"] + [os.path.basename(f) + e for f in (f1, f2) for e in (".correct.fa.gz", ".correct.stat")]
                                                     + ["reads_1.fq.gz.correct.fa.gz" + e for e in (".pair.fa.gz", ".single.fa.gz", ".pair.single.stat")])
            res[name] = stat.decode().split()[2::3]
    with tempfile.TemporaryDirectory() as tmp:   # mate file 2 is one record short
        f1, f2 = os.path.join(tmp, "reads_1.fq.gz"), os.path.join(tmp, "reads_2.fq")
        shutil.copy(os.path.join(PR.CORRECT, "reads.fq.gz"), f1)
        lines = gzip.open(f1, "rb").read().split(b"\n")
        open(f2, "wb").write(b"\n".join(lines[:-5]) + b"\n")
        with open(os.path.join(tmp, "reads.lib"), "w") as f:
            f.write("%s\n%s\n" % (f1, f2))
        r = subprocess.run([EXE, "-k", "13", "-f", "1", "-j", "1", os.path.join(PR.CORRECT, "table.cz"), os.path.join(tmp, "reads.lib")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "hold different numbers of records" in r.stderr, (r.returncode, r.stderr[-2000:])
        res["different_record_counts"] = r.returncode
    return res


# ---- hand-offs ---------------------------------------------------------------------------------------------------------------------------
def mates_150(n_pairs, seed, emptied=0.1):
    """two batches of 150-base reads of one synthetic genome, about `emptied` of the reads of either emptied"""
    from oracle import oracle_py as O
    bases, offsets = O.synth_reads(O.synth_params(20000, 150, cfg=1), seed * 100000, 2 * n_pairs)
    raw = np.ascontiguousarray(bases, dtype=np.uint8).tobytes()
    reads = [raw[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]
    rng = np.random.default_rng(seed)
    reads = [b"" if rng.random() < emptied else r for r in reads]
    return PR.pack(reads[0::2]), PR.pack(reads[1::2])


def host_reads(want, which):
    bases, _, off, _ = want[0][which]
    return np.ascontiguousarray(bases[:int(off[-1])]), off


def graph():
    from dbg_assembly_amd import capi
    from clean_compact_gpu_steps import graph_args, result_of, same
    (b1, o1), (b2, o2) = mates_150(3000, 1)
    want = PR.split(b1, o1, b2, o2)
    res = {}
    with capi.Pairer() as p:
        info = p.split(b1, o1, b2, o2)
        assert info["pair_reads"] > 0 and info["single_reads"] > 0 and info["pair_reads"] + info["single_reads"] < 6000
        for engine in ("direct", "partition"):
            with capi.Graph(**graph_args(capi, engine, 6000)) as g:
                g.push_pairs(p, capi.PAIR_PAIRED)
                g.push_pairs(p, capi.PAIR_SINGLE)
                new = result_of(g)
                digest_new = g.digest()
            with capi.Graph(**graph_args(capi, engine, 6000)) as g:
                g.push_reads(*host_reads(want, PR.PAIRED))
                g.push_reads(*host_reads(want, PR.SINGLE))
                old = result_of(g)
                digest_old = g.digest()
            same(new, old, engine)
            assert digest_new == digest_old, engine
            res[engine] = {"reads": new[0][0], "nodes": new[0][2]}
    assert res["direct"] == res["partition"] and res["direct"]["reads"] == info["pair_reads"] + info["single_reads"]
    return res


def mapper():
    """Mapper.map_device on the PAIR batch where it lies against Mapper.map on its host copy.  Mates are the reads of a golden case,
    the second batch the same reads rotated by one with a few emptied by hand; the second case holds a read beyond the LDS slice"""
    from dbg_assembly_amd import capi
    import map_restatement as MR
    cases = os.path.join(ROOT, "tests", "golden", "map_cases")
    _, contigs = MR.read_contig_file(os.path.join(cases, "contigs.fa"), 0)
    reads = [r.encode() for _, r in MR.records_map_reads(os.path.join(cases, "pe_1.fq.gz"), 1)]
    long_read = max(contigs, key=len)[:1500].encode()
    if len(long_read) <= 1024:
        long_read = (b"".join(reads))[:1500]
    assert len(long_read) > 1024
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Pairer() as p, \
            capi.Mapper(k=31, s=5, r=30, identity=0.97, second_alignment=False) as m:
        m.set_contigs(contigs)
        for name, first in (("reads", reads), ("with_a_long_read", reads[:50] + [long_read] + reads[50:])):
            second = PR.rotate(first)
            second = [b"" if i % 17 == 3 else r for i, r in enumerate(second)]
            first = [b"" if i % 23 == 5 else r for i, r in enumerate(first)]
            (b1, o1), (b2, o2) = PR.pack(first), PR.pack(second)
            info = p.split(b1, o1, b2, o2)
            d_b, _, d_o, n, nb = p.device(capi.PAIR_PAIRED)
            got = m.map_device(d_b, d_o, n, nb, info["max_len"])
            st_dev = m.batch_stats()
            bases, _, off, _ = p.results(capi.PAIR_PAIRED)
            want = m.map(bases, off)
            st_host = m.batch_stats()
            assert n == info["pair_reads"] > 0 and info["single_reads"] > 0
            assert got.tobytes() == want.tobytes(), name
            for f in ("reads", "by_lds", "by_long", "skipped", "windows_probed"):
                assert st_dev[f] == st_host[f], (name, f, st_dev, st_host)
            if name == "with_a_long_read":
                assert st_dev["by_long"] > 0 and info["max_len"] == len(long_read)
                # a max_len below the longest read is refused, not served from behind the identity table
                try:
                    m.map_device(d_b, d_o, n, nb, 1024)
                    res["max_len_too_small"] = capi.OK
                except capi.DbgkError as e:
                    res["max_len_too_small"] = e.status
            res[name] = {"reads": n, "mapped": int((got["contig"][:, 0] != -1).sum()), "by_long": st_dev["by_long"]}
            assert res[name]["mapped"] > 0
    return res


def reuse():
    """one Pairer, three splits back to back -- a batch, a smaller one, a larger one that regrows every buffer -- each pushed into the
    graph at once, the next split started without a sync of the graph: the graph equals the one built from the host copies"""
    from dbg_assembly_amd import capi
    from clean_compact_gpu_steps import graph_args, result_of, same
    batches = [mates_150(1500, 2), mates_150(400, 3), mates_150(9000, 4)]
    wants = [PR.split(b1, o1, b2, o2) for (b1, o1), (b2, o2) in batches]
    n = 2 * (1500 + 400 + 9000)
    with capi.Graph(**graph_args(capi, "partition", n)) as g, capi.Pairer() as p:
        for ((b1, o1), (b2, o2)), want in zip(batches, wants):
            info = p.split(b1, o1, b2, o2)
            assert {f: info[f] for f in PR.COUNTERS} == want[1]
            g.push_pairs(p, capi.PAIR_PAIRED)
            g.push_pairs(p, capi.PAIR_SINGLE)
        new = result_of(g)
    with capi.Graph(**graph_args(capi, "partition", n)) as g:
        for want in wants:
            g.push_reads(*host_reads(want, PR.PAIRED))
            g.push_reads(*host_reads(want, PR.SINGLE))
        old = result_of(g)
    same(new, old, "reuse")
    return {"reads": new[0][0], "nodes": new[0][2]}


def status_of(call):
    from dbg_assembly_amd import capi
    try:
        call()
    except capi.DbgkError as e:
        return e.status
    return capi.OK


def states():
    from dbg_assembly_amd import capi
    (b1, o1), (b2, o2) = mates_150(100, 6)
    res = {}
    with capi.Graph(k=31, table_slots=capi.find_next_prime_ref(100000), engine=capi.ENGINE_DIRECT) as g, capi.Pairer() as p:
        res["results_before_a_split"] = status_of(lambda: p.results(capi.PAIR_PAIRED))
        res["device_before_a_split"] = status_of(lambda: p.device(capi.PAIR_SINGLE))
        res["push_before_a_split"] = status_of(lambda: g.push_pairs(p, capi.PAIR_PAIRED))
        p.split(b1, o1, b2, o2)
        d_b, _, d_o, n, nb = p.device(capi.PAIR_PAIRED)
        res["which_out_of_range"] = status_of(lambda: p.device(2))
        res["misaligned_plane"] = status_of(lambda: p.split_device(d_b + 4, d_o, d_b, d_o, 1))
        res["own_output_as_input"] = status_of(lambda: p.split_device(d_b, d_o, d_b, d_o, n))
        res["qualities_for_one_mate_only"] = capi.lib().dbgk_pair_split_from(p._h, b1.ctypes.data, b1.ctypes.data, o1.ctypes.data, b2.ctypes.data, None,
                                                                             o2.ctypes.data, 100, ctypes.byref(capi.PairInfo()))
        bad = o1.copy()
        bad[0] = 1
        res["offsets_that_do_not_start_at_0"] = status_of(lambda: p.split(b1, bad, b2, o2))
        res["results_after_a_refused_split"] = status_of(lambda: p.results(capi.PAIR_PAIRED))
        p.split(b1, o1, b2, o2)
        q = np.zeros(max(nb, 1), dtype=np.uint8)
        res["quality_plane_of_an_output_without_one"] = capi.lib().dbgk_pair_results(p._h, 0, None, q.ctypes.data, None, None)
        res["results_with_no_pointer"] = capi.lib().dbgk_pair_results(p._h, 0, None, None, None, None)
        g.push_pairs(p, capi.PAIR_PAIRED)
        g.finalize()
        res["push_into_a_finalized_handle"] = status_of(lambda: g.push_pairs(p, capi.PAIR_SINGLE))
    return res


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "many": many, "subrange": subrange, "goldens": goldens, "cli": cli, "graph": graph, "mapper": mapper,
                      "reuse": reuse, "states": states}[sys.argv[1]]()))
