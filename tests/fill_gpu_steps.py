"""GPU steps of tests/test_fill_gpu.py, each run in a child process of its own under a time limit:
    python tests/fill_gpu_steps.py cases | pipeline | large | emit
Prints one JSON line of findings; exits non-zero on a mismatch."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fill_restatement as FR  # noqa: E402
import link_restatement as LR  # noqa: E402
from link_gpu_steps import same_table  # noqa: E402

CASES = os.path.join(ROOT, "tests", "golden", "fill_cases")
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")


def check_against(g, res, lens, seqs, what):
    """a built capi.GapFiller against the restatement's result: table, gap statistics, layout, consensus, emitted bytes"""
    from dbg_assembly_amd import capi  # noqa: F401
    same_table(g.table(), res["table"], what)
    st = g.gap_stats()
    want = sorted(res["stats"].items())
    assert len(st) == len(want), (what, len(st), len(want))
    got_rows = np.stack([st[f] for f in ("contig_lo", "contig_hi", "mode", "mode_freq", "total_freq", "variance")], axis=1).astype(np.int64)
    want_rows = np.array([[k[0], k[1], v[0], v[1], v[2], v[3]] for k, v in want], dtype=np.int64).reshape(-1, 6)
    assert np.array_equal(got_rows, want_rows), (what, "gap statistics")
    summ = g.resolve()
    c = res["counters"]
    assert (summ["lowfreq"], summ["repeat_nodes"], summ["deleted"], summ["scaffolds"]) == (c["lowfreq"], c["repeat"], c["deleted"], c["scaffolds"]), (summ, c)
    scaf_first, items, gaps, repeats, cons = g.layout()
    assert repeats.tolist() == res["repeats"], what
    assert np.array_equal(np.diff(scaf_first.astype(np.int64)), [len(it) for it in res["layout"]]), what
    flat = [it for its in res["layout"] for it in its]
    assert len(flat) == len(items)
    cons_b = cons.tobytes()
    host_path = 0
    for it, (c_, rev, length, gi, off) in zip(flat, items.tolist()):
        if it[0] == "ctg":
            assert (c_, rev, length) == (it[1], it[2], it[3]), (what, it)
        else:
            G = gaps[gi]
            assert c_ == -1 and (int(G["mode"]), int(G["mode_freq"]), int(G["total_freq"]), int(G["variance"])) == it[1:5], (what, it, G)
            assert length == max(it[1], 0)
            if it[1] > 0:
                assert cons_b[off:off + length] == it[5].encode("latin-1"), (what, it[:5])
                assert np.float32(G["identity"]).tobytes() == np.float32(it[6]).tobytes(), (what, it[:5], float(G["identity"]), float(it[6]))
                host_path += int(G["host_path"])
    if seqs is not None:
        got = g.emit([s.encode("latin-1") for s in seqs], items).tobytes()
        want_seq = "".join(FR.emit_string(seqs, its) for its in res["layout"]).encode("latin-1")
        assert got == want_seq, (what, "emit")
    return summ, host_path


def cases():
    """capi.GapFiller on every fixture == the restatement (which equals the reference program there), texts included"""
    from dbg_assembly_amd import capi
    out = {}
    for case in FR.golden_cases(CASES):
        P, names, seqs, recs, files, reads = FR.load_case(CASES, case)
        lens = [len(s) for s in seqs]
        want = LR.expected_outputs(CASES, case)
        res = FR.run(P, names, lens, recs, files, seqs, reads, prefix=case["prefix"])
        with capi.GapFiller(P.n) as g:
            g.set_contigs(lens)
            g.set_reads([r.encode("latin-1") for r in reads])
            for r in recs:
                g.add_records(r)
            g.build()
            summ, host_path = check_against(g, res, lens, seqs, case["name"])
            pos, rep = g.pos_tabs(names)
            texts = {"contig_R.links.all": g.links_text(0), "contig_R.links.uniq": g.links_text(1), "contig_R.pos.tab": pos,
                     "contig_R.repeat.pos.tab": rep}
        for k, t in texts.items():
            assert t == want["%s.%s" % (case["prefix"], k)], (case["name"], k)
        if P.n <= 3:
            assert host_path >= 1                      # the gap with lower-case bytes took the counted path, the one with N did not
        out[case["name"]] = {"gaps": summ["gaps"], "filled": summ["filled"], "host_path": host_path}
    # a spanning read shorter than its slice: DBGK_ERR_ARG, whatever else the job holds
    case = FR.golden_cases(CASES)[1]
    P, names, seqs, recs, files, reads = FR.load_case(CASES, case)
    short = [r[:30] for r in reads]
    with capi.GapFiller(P.n) as g:
        g.set_contigs([len(s) for s in seqs])
        g.set_reads([r.encode("latin-1") for r in short])
        for r in recs:
            g.add_records(r)
        g.build()
        try:
            g.resolve()
        except capi.DbgkError as e:
            assert e.status == capi.ERR_ARG
        else:
            raise AssertionError("a slice outside its read was accepted")
    return out


def pipeline():
    """bin/map_reads -> bin/link_contig on a generated genome returns the source sequence across the filled gaps; and
    GapFiller.add_hits on capi.Mapper's hits == add_records on the parsed 2ctg text of the same reads"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(21)
    genome = "".join("ACGT"[v] for v in rng.integers(0, 4, 9000))
    cuts = [(0, 1500), (1520, 3000), (3035, 4490), (4500, 6000), (6012, 7500), (7540, 9000)]   # gaps 20, 35, 10, 12, 40
    contigs = [genome[a:b] for a, b in cuts]
    contigs[2] = LR.reverse_complement(contigs[2])      # one contig comes on the other strand
    reads = []
    for k, (a, b) in enumerate(cuts[:-1]):
        for j in range(6):                              # six reads over every junction, alternately of either strand
            s = b - 120 - 10 * j
            r = genome[s:s + 300]
            reads.append(LR.reverse_complement(r) if j % 2 else r)
    for s in range(100, 8600, 700):                     # and reads inside contigs or nowhere
        reads.append(genome[s:s + 300])
    reads.append("".join("ACGT"[v] for v in rng.integers(0, 4, 300)))
    work = tempfile.mkdtemp()
    with open(os.path.join(work, "contigs.fa"), "w") as f:
        for c, s in enumerate(contigs):
            f.write(">ctg_%d\n%s\n" % (2 * c + 1, s))
    with open(os.path.join(work, "reads.fa"), "w") as f:
        for k, r in enumerate(reads):
            f.write(">read_%d\n%s\n" % (k, r))
    open(os.path.join(work, "reads.lib"), "w").write("reads.fa\n")
    r = subprocess.run([os.path.join(BIN, "map_reads"), "-f", "0", "-o", "./", "contigs.fa", "reads.lib"], cwd=work, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(BIN, "link_contig"), "-o", "out", "contigs.fa", "reads.lib.map_reads.2ctg.lib"], cwd=work,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    fa = open(os.path.join(work, "out.contig_R.seq.fa")).read().split("\n")
    assert len(fa) == 3 and "fragment_num:6" in fa[0], fa[0]
    assert fa[1] in (genome, LR.reverse_complement(genome)), "link_contig did not return the source sequence"
    # the same reads through the bindings
    lib_files = LR.read_lib(open(os.path.join(work, "reads.lib.map_reads.2ctg.lib")).read())
    text = gzip.open(os.path.join(work, lib_files[0])).read().decode("latin-1")
    index = {"read_%d" % k: k for k in range(len(reads))}
    recs = FR.parse_2ctg(text, len(contigs), index)
    assert len(recs) >= 20 and len(index) == len(reads)     # (at least four of the six reads of every junction)
    lens = [len(c) for c in contigs]
    with capi.Mapper(second_alignment=True) as m:
        m.set_contigs([c.encode() for c in contigs])
        hits = m.map_sequences([q.encode() for q in reads])
    got = []
    for mode in ("hits", "records"):
        with capi.GapFiller(3) as g:
            g.set_contigs(lens)
            g.set_reads([q.encode() for q in reads])
            if mode == "hits":
                g.add_hits(hits[:7], 0)
                g.add_hits(hits[7:], 7)
            else:
                g.add_records(recs)
            g.build()
            t = g.table()
            summ = g.resolve()
            got.append((t, g.gap_stats().tolist(), [x.tolist() for x in g.layout()], summ, g.timing()))
    same_table(got[0][0], (got[1][0][0], got[1][0][1], {k: int(v) for k, v in got[1][0][2].items()}), "hits")
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2] and got[0][3] == got[1][3]
    assert got[0][4]["records"] == len(reads) and got[1][4]["records"] == len(recs) and got[0][4]["pooled"] == len(recs)
    assert sorted(s[2] for s in got[0][1]) == [10, 12, 20, 35, 40]
    return {"reads": len(reads), "two_contig_reads": len(recs), "length": len(fa[1])}


def large_job(rng, n_contigs, n, n_reads, read_len):
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads_arr = alphabet[rng.integers(0, 4, (n_reads, read_len))]
    reads_arr[rng.random((n_reads, read_len)) < 0.002] = ord("N")
    reads = [row.tobytes().decode() for row in reads_arr]
    lens = rng.integers(60, 400, n_contigs).astype(np.uint32)
    recs = np.zeros(n, dtype=FR.REC_DTYPE)
    c1 = rng.integers(0, n_contigs - 4, n)
    c1 -= (c1 % 4 == 3)                                 # chains of four contigs: no link leaves a contig whose index is 3 mod 4
    c2 = c1 + 1
    noise = rng.random(n) < 0.1                         # a tenth of the records anywhere
    c2[noise] = (c1[noise] + rng.integers(2, 50, int(noise.sum()))) % n_contigs
    hot = rng.random(n) < 0.05                          # a twentieth on 40 pairs: thousands of spanning reads each
    c1[hot] = rng.integers(0, 40, int(hot.sum())) * 1000
    c2[hot] = c1[hot] + 1
    base = ((c1 * 2654435761) % 61).astype(np.int64) - 25   # the pair's gap, -25 .. 35
    gap = np.where(rng.random(n) < 0.75, base, base + rng.integers(-3, 4, n))
    recs["read"] = rng.integers(0, n_reads, n)
    recs["read_len"] = read_len
    recs["align1_end"] = rng.integers(30, 60, n)
    recs["align2_start"] = recs["align1_end"] + gap + 1
    recs["contig1"], recs["contig2"] = c1, c2
    d = np.frombuffer(b"FFFFFFFFFFFFFFFN", dtype=np.uint8)
    recs["direct1"], recs["direct2"] = d[rng.integers(0, 16, n)], d[rng.integers(0, 16, n)]
    swap = rng.random(n) < 0.5                          # half of the reads are of the other strand: R, R with the contigs exchanged
    ok = swap & (recs["direct1"] == ord("F")) & (recs["direct2"] == ord("F"))
    a, b = recs["contig1"].copy(), recs["contig2"].copy()
    recs["contig1"][ok], recs["contig2"][ok] = b[ok], a[ok]
    recs["direct1"][ok] = ord("R")
    recs["direct2"][ok] = ord("R")
    return lens, recs, reads


def large():
    """3 M records over 100 k contigs in unequal batches == the restatement: table, statistics, layout, consensus"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(12)
    n_contigs, n = 100000, 3000000
    lens, recs, reads = large_job(rng, n_contigs, n, 40000, 128)
    P = FR.Params(n=3)
    names = ["ctg_%d" % (2 * c + 1) for c in range(n_contigs)]
    res = FR.run(P, names, lens, [recs], ["x"], None, reads)
    with capi.GapFiller(P.n) as g:
        g.set_contigs(lens)
        g.set_reads([r.encode() for r in reads])
        cuts = [0, 1, 1, 777777, 777777 + 1500001, n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            g.add_records(recs[a:b])
        g.build()
        summ, host_path = check_against(g, res, lens, None, "large")
        st = g.timing()
    gaps = [it for its in res["layout"] for it in its if it[0] == "gap"]
    return {"records": n, "pooled": st["pooled"], "links": st["links"], "scaffolds": summ["scaffolds"], "repeat_nodes": summ["repeat_nodes"],
            "gaps": len(gaps), "filled": sum(g[1] > 0 for g in gaps), "cut": sum(g[1] <= 0 for g in gaps),
            "max_span": max(g[2] for g in gaps), "host_path": host_path,
            **{k: st[k] for k in ("ms_orient", "ms_sort", "ms_table", "ms_gapstat", "ms_consensus", "cons_bytes", "span_bytes")}}


def emit():
    """an emit layout with whole, cut and reversed contigs of 0 bytes up to more than 2^20 and spliced gap bytes == the restatement"""
    from dbg_assembly_amd import capi
    case = FR.golden_cases(CASES)[0]
    P, names, seqs, recs, files, reads = FR.load_case(CASES, case)
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNnRYKMSWBDHVryx-*", dtype=np.uint8)
    extra = [alphabet[rng.integers(0, len(alphabet), n)].tobytes().decode() for n in (1, 7, 8, 9, 63, 65, 4097, (1 << 20) + 3, 300001)]
    with capi.GapFiller(P.n) as g:
        g.set_contigs([len(s) for s in seqs])
        g.set_reads([r.encode("latin-1") for r in reads])
        for r in recs:
            g.add_records(r)
        g.build()
        g.resolve()
        _, items, gaps, _, cons = g.layout()
        filled = [it for it in items.tolist() if it[0] < 0 and it[2] > 0]
        assert len(filled) >= 5
        contigs = seqs + extra + [""]
        lay, want = [], []
        for _ in range(600):
            if rng.random() < 0.3:
                it = filled[int(rng.integers(0, len(filled)))]
                lay.append(tuple(it))
                want.append(cons[it[4]:it[4] + it[2]].tobytes().decode("latin-1"))
            else:
                c = int(rng.integers(0, len(contigs)))
                if len(contigs[c]) > 70000 and rng.random() < 0.6:
                    c = int(rng.integers(0, len(seqs)))
                rev = int(rng.integers(0, 2))
                full = len(contigs[c])
                length = full if rng.random() < 0.5 else int(rng.integers(0, full + 1))
                lay.append((c, rev, length, -1, 0))
                want.append((LR.reverse_complement(contigs[c]) if rev else contigs[c])[:length])
        got = g.emit([c.encode("latin-1") for c in contigs], np.array(lay, dtype=capi.FILL_ITEM_DTYPE)).tobytes()
        none = g.emit([c.encode("latin-1") for c in contigs], np.zeros(0, dtype=capi.FILL_ITEM_DTYPE)).tobytes()
        for bad in ((0, 0, len(contigs[0]) + 1, -1, 0), (-1, 0, 5, 0, len(cons) - 4), (len(contigs), 0, 0, -1, 0)):
            try:
                g.emit([c.encode("latin-1") for c in contigs], np.array([bad], dtype=capi.FILL_ITEM_DTYPE))
            except capi.DbgkError as e:
                assert e.status == capi.ERR_ARG
            else:
                raise AssertionError("a bad item was accepted: %r" % (bad,))
        st = g.timing()
    want = "".join(want).encode("latin-1")
    assert len(got) == len(want) and got == want and none == b""
    return {"bytes": len(want), "items": len(lay), "ms_emit": st["ms_emit"]}


if __name__ == "__main__":
    print(json.dumps({"cases": cases, "pipeline": pipeline, "large": large, "emit": emit}[sys.argv[1]]()))
