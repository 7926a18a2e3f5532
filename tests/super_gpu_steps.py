"""GPU steps of tests/test_super_gpu.py, each run in a child process of its own under a time limit:
    python tests/super_gpu_steps.py cases | pipeline | random
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
import super_restatement as SR  # noqa: E402
from link_gpu_steps import same_table  # noqa: E402

CASES = os.path.join(ROOT, "tests", "golden", "super_cases")
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")


def device_reads(reads):
    """the reads as the program hands them to the device: those no file holds get indices behind the others; -> list, index map"""
    present = [k for k, r in enumerate(reads) if r is not None]
    absent = [k for k, r in enumerate(reads) if r is None]
    remap = np.zeros(len(reads), dtype=np.int32)
    remap[present + absent] = np.arange(len(reads))
    return [reads[k].encode("latin-1") for k in present], remap


def check_against(g, res, seqs, what):
    """a built capi.SuperLinker against the restatement's result: table, statistics, layout, slice records, slice bytes, emit"""
    same_table(g.table(), res["table"], what)
    st = g.gap_stats()
    want = sorted(res["stats"].items())
    got_rows = np.stack([st[f] for f in ("contig_lo", "contig_hi", "mean", "min", "max", "total", "variance")], axis=1).astype(np.int64)
    want_rows = np.array([[k[0], k[1]] + list(v[:5]) for k, v in want], dtype=np.int64).reshape(-1, 7)
    assert np.array_equal(got_rows, want_rows), (what, "gap statistics")
    summ = g.resolve()
    c = res["counters"]
    assert (summ["lowfreq"], summ["interleave"], summ["repeat_nodes"], summ["deleted"], summ["scaffolds"]) == \
        (c["lowfreq"], c["interleave"], c["repeat"], c["deleted"], c["scaffolds"]), (what, summ, c)
    scaf_first, items, junctions, repeats = g.layout()
    assert repeats.tolist() == res["repeats"], what
    assert np.array_equal(np.diff(scaf_first.astype(np.int64)), [len(it) for it in res["layout"]]), what
    flat = [it for its in res["layout"] for it in its]
    assert len(flat) == len(items) and len(junctions) == len(res["junctions"]) == summ["junctions"]
    J = iter(junctions.tolist())
    for it, (c_, v) in zip(flat, items.tolist()):
        if it[0] == "ctg":
            assert (c_, v) == (it[1], it[2]), (what, it)
        else:
            j = next(J)
            assert c_ == -1 and v == it[2], (what, it)
            # left, right, mean, min, max, total, variance, n_written, gap_id
            assert tuple(j[2:9]) == (it[7], it[3], it[4], it[5], it[6], it[2], it[1]), (what, it, j)
    slices, data = g.slices()
    data = data.tobytes()
    by_id = {int(j["gap_id"]): j for j in junctions}
    at = lines = 0
    for want_j in res["junctions"]:
        j = by_id[want_j["gap_id"]]
        assert (int(j["left_contig"]), int(j["right_contig"])) == (want_j["left"], want_j["right"]), (what, want_j["gap_id"])
        first, n = int(j["first_slice"]), int(j["n_slices"])
        ws = want_j["slices"]
        assert n == len(ws) and int(j["median"]) == want_j["median"], (what, want_j["gap_id"])
        got = slices[first:first + n]
        assert got["record"].tolist() == [s[1] for s in ws], (what, want_j["gap_id"], "sorted order")
        assert got["length"].tolist() == [s[0] for s in ws] and got["reversed"].tolist() == [s[2] for s in ws]
        assert got["kept"].tolist() == [s[3] for s in ws], (what, want_j["gap_id"], "kept")
        assert int(j["n_kept"]) == sum(s[3] > 0 for s in ws)
        order = [want_j["median"]] + [k for k in range(n) if k != want_j["median"] and ws[k][3]]
        for k in order:                                # back to back in the order gap.data lists them
            assert int(got["offset"][k]) == at, (what, want_j["gap_id"], k)
            assert data[at:at + ws[k][0]] == ws[k][4].encode("latin-1"), (what, want_j["gap_id"], k, "slice bytes")
            at += ws[k][0]
            lines += 1
    assert at == len(data) == summ["slice_bytes"] and lines == summ["lines"] and len(slices) == summ["slices"]
    if seqs is not None:
        got = g.emit([s.encode("latin-1") for s in seqs], items).tobytes()
        want_seq = "".join(SR.emit_string(seqs, its) for its in res["layout"]).encode("latin-1")
        assert got == want_seq, (what, "emit")
    return summ


def linker(P, lens, reads, recs_list):
    from dbg_assembly_amd import capi
    dev, remap = device_reads(reads)
    g = capi.SuperLinker(P.n)
    g.set_contigs(lens)
    g.set_reads(dev)
    for r in recs_list:
        r = r.copy()
        r["read"] = remap[r["read"]]
        g.add_records(r)
    g.build()
    return g


def cases():
    """capi.SuperLinker on every fixture == the restatement (which equals the reference program there); a read that is too short
    and a read that is missing are DBGK_ERR_ARG with the record named"""
    from dbg_assembly_amd import capi
    out = {}
    for case in SR.golden_cases(CASES):
        P, names, seqs, recs, files, reads = SR.load_case(CASES, case)
        lens = [len(s) for s in seqs]
        res = SR.run(P, names, lens, recs, files, seqs, reads, prefix=case["prefix"])
        with linker(P, lens, reads, recs) as g:
            summ = check_against(g, res, seqs, case["name"])
            want = LR.expected_outputs(CASES, case)
            for stage, kind in ((0, "supertig.links.all"), (1, "supertig.links.uniq")):
                assert g.links_text(stage) == want["%s.%s" % (case["prefix"], kind)], (case["name"], kind)
        out[case["name"]] = {k: summ[k] for k in ("junctions", "slices", "lines", "slice_bytes")}
    case = SR.golden_cases(CASES)[1]
    P, names, seqs, recs, files, reads = SR.load_case(CASES, case)
    lens = [len(s) for s in seqs]
    for what in ("short", "missing"):
        bad = list(reads)
        victim = int(recs[0][0]["read"])               # the first record spans 0+ -> 1+, a junction of the layout
        bad[victim] = bad[victim][:100] if what == "short" else None
        try:
            SR.run(P, names, lens, recs, files, seqs, bad)
        except SR.BadSlice as e:
            want_bad = (e.record, e.left, e.right)
        else:
            raise AssertionError("the restatement accepted a %s read" % what)
        with linker(P, lens, bad, recs) as g:
            try:
                g.resolve()
            except capi.DbgkError as e:
                assert e.status == capi.ERR_ARG and (e.bad["bad_record"], e.bad["bad_left"], e.bad["bad_right"]) == want_bad, (what, e.bad, want_bad)
            else:
                raise AssertionError("a %s read was accepted" % what)
    return out


def pipeline():
    """bin/map_reads -> bin/link_supertig on three contigs cut from one source returns the source with every gap as N x its mean;
    and SuperLinker.add_hits on capi.Mapper's hits == add_records on the parsed 2ctg text of the same reads"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(33)
    genome = "".join("ACGT"[v] for v in rng.integers(0, 4, 12000))
    cuts = [(0, 4000), (4040, 8000), (8130, 12000)]     # gaps 40 and 130
    contigs = [genome[a:b] for a, b in cuts]
    contigs[1] = LR.reverse_complement(contigs[1])      # one contig comes on the other strand
    reads = []
    for k, (a, b) in enumerate(cuts[:-1]):
        for j in range(20):                             # twenty 1400-bp reads over every junction, alternately of either strand
            s = b - 800 + 12 * j
            r = genome[s:s + 1400]
            reads.append(LR.reverse_complement(r) if j % 2 else r)
    for s in (500, 5000, 9500):                         # and reads inside contigs or nowhere
        reads.append(genome[s:s + 1400])
    reads.append("".join("ACGT"[v] for v in rng.integers(0, 4, 1400)))
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
    r = subprocess.run([os.path.join(BIN, "link_supertig"), "-o", "out", "contigs.fa", "reads.lib.map_reads.2ctg.lib"], cwd=work,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    fa = open(os.path.join(work, "out.supertig.seq.fa")).read().split("\n")
    assert len(fa) == 3 and "fragment_num:3" in fa[0], fa[0]
    gaps = [l.split("\t") for l in open(os.path.join(work, "out.supertig.pos.tab")).read().split("\n") if l.startswith("\tgap")]
    widths = [int(t[4]) for t in gaps]
    assert len(widths) == 2 and min(widths) > 0
    forward = genome[0:4000] + "N" * widths[0] + genome[4040:8000] + "N" * widths[1] + genome[8130:12000]
    backward = LR.reverse_complement(genome[8130:12000]) + "N" * widths[0] + LR.reverse_complement(genome[4040:8000]) + "N" * widths[1] + \
        LR.reverse_complement(genome[0:4000])
    assert fa[1] in (forward, backward), "link_supertig did not return the source sequence"
    # the same reads through the bindings
    lib_files = LR.read_lib(open(os.path.join(work, "reads.lib.map_reads.2ctg.lib")).read())
    text = gzip.open(os.path.join(work, lib_files[0])).read().decode("latin-1")
    index = {"read_%d" % k: k for k in range(len(reads))}
    recs = FR.parse_2ctg(text, len(contigs), index)
    assert len(recs) >= 30 and len(index) == len(reads)
    lens = [len(c) for c in contigs]
    with capi.Mapper(second_alignment=True) as m:
        m.set_contigs([c.encode() for c in contigs])
        hits = m.map_sequences([q.encode() for q in reads])
    got = []
    for mode in ("hits", "records"):
        with capi.SuperLinker(3) as g:
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
            sl, data = g.slices()
            # (a slice's record counts the reads in one mode and the lines in the other: compared through the read)
            rd = sl["record"].tolist() if mode == "hits" else recs["read"][sl["record"].astype(np.int64)].tolist()
            got.append((t, g.gap_stats().tolist(), [x.tolist() for x in g.layout()[:2]], summ, g.timing(), rd,
                        sl[["length", "reversed", "kept"]].tolist(), data.tobytes(), [j[2:] for j in g.layout()[2].tolist()]))
    same_table(got[0][0], (got[1][0][0], got[1][0][1], {k: int(v) for k, v in got[1][0][2].items()}), "hits")
    for k in (1, 2, 3, 5, 6, 7, 8):
        assert got[0][k] == got[1][k], ("hits against records", k)
    assert got[0][4]["records"] == len(reads) and got[1][4]["records"] == len(recs) and got[0][4]["pooled"] == len(recs)
    means = sorted(s[2] for s in got[0][1])
    assert sorted(widths) == means
    return {"reads": len(reads), "two_contig_reads": len(recs), "length": len(fa[1]), "gaps": widths}


RUNS = (1, 2, 255, 256, 257, 1100)                      # records per pair: runs begin and end on either side of a 256-thread block
LENGTHS = (0, 1, 63, 64, 65, 499, 500, 501)             # slice lengths of clamped reads


def random_job(rng, n_contigs=300, n_target=4000):
    """chains of three contigs; per pair a run of records in random file order, half from the other strand, some of wrong direction,
    gaps around a base of the pair's own (negative ones among them); a read of its own per record, cut for the slice length wanted"""
    lens = rng.integers(300, 900, n_contigs).astype(np.uint32)
    pairs = [(c, c + 1) for c in range(n_contigs - 1) if c % 3 != 2]
    runs = list(RUNS) + [int(x) for x in rng.integers(1, 22, len(pairs) - len(RUNS))]
    rows, read_lens = [], []
    special = list(LENGTHS) * 6
    for p, ((x, y), n) in enumerate(zip(pairs, runs)):
        base = int(rng.integers(-40, 60)) if p % 4 else -int(rng.integers(2, 30))
        for k in range(n):
            gap = base + int(rng.integers(-3, 4))
            if p == 7 and k == 0:
                gap = 4000                              # a slice above 4096 bytes
            start = int(rng.integers(0, 40))            # where the slice is to begin
            a1e = start + 251 + max(-gap, 0)
            a2s = a1e + gap + 1
            g = max(gap, 0)
            pos = LR.c_div(a1e + a2s, 2) - 250 - g // 2
            assert pos >= 0
            want = g + 500
            if special and k % 3 == 1 and n > 2:
                want = special.pop()
            read_lens.append(pos + want + (int(rng.integers(0, 50)) if want == g + 500 else 0))
            swap = rng.random() < 0.5
            d1, d2 = ("R", "R") if swap else ("F", "F")
            if rng.random() < 0.03:
                d1 = "N"
            c1, c2 = (y, x) if swap else (x, y)
            rows.append((len(rows), read_lens[-1], a1e, a2s, c1, c2, ord(d1), ord(d2), (0, 0)))
    assert not special
    order = rng.permutation(len(rows))
    recs = np.array([rows[k] for k in order], dtype=SR.REC_DTYPE)
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTNacgtnRY", dtype=np.uint8)
    reads = [alphabet[rng.integers(0, len(alphabet), n)].tobytes().decode() for n in read_lens]
    return lens, recs, reads


def random():
    """a job sized for the kernels == the restatement: statistics of runs that straddle blocks, slices of every awkward length"""
    rng = np.random.default_rng(8)
    lens, recs, reads = random_job(rng)
    P = SR.Params(n=1)
    names = ["ctg_%d" % (2 * c + 1) for c in range(len(lens))]
    seqs = ["".join("ACGT"[v] for v in rng.integers(0, 4, int(n))) for n in lens]
    cuts = [0, 1, 1, 1500, len(recs)]
    parts = [recs[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    res = SR.run(P, names, lens, parts, ["x"], seqs, reads)
    with linker(P, lens, reads, parts) as g:
        summ = check_against(g, res, seqs, "random")
        st = g.timing()
    totals = sorted(v[3] for v in res["stats"].values())
    lengths = {s[0] for j in res["junctions"] for s in j["slices"]}
    assert set(RUNS) <= set(totals) and set(LENGTHS) <= lengths and max(lengths) > 4096
    assert any(v[0] < 0 for v in res["stats"].values())
    flipped = [s[2] for j in res["junctions"] for s in j["slices"]]
    assert 0.3 < sum(flipped) / len(flipped) < 0.7
    return {"records": len(recs), "pairs": len(res["stats"]), "junctions": summ["junctions"], "slices": summ["slices"],
            "slice_bytes": summ["slice_bytes"], "ms_gapstat": st["ms_gapstat"], "ms_slices": st["ms_slices"]}


if __name__ == "__main__":
    print(json.dumps({"cases": cases, "pipeline": pipeline, "random": random}[sys.argv[1]]()))
