"""GPU steps of tests/test_link_gpu.py, each run in a child process of its own under a time limit:
    python tests/link_gpu_steps.py ecoli | hits | large | emit
Prints one JSON line of findings; exits non-zero on a mismatch."""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import link_restatement as LR  # noqa: E402
import map_restatement as MR  # noqa: E402

CASES = os.path.join(ROOT, "tests", "golden", "link_cases")
MAP_CASES = os.path.join(ROOT, "tests", "golden", "map_cases")


def same_table(got, want, what):
    for g, w, name in zip(got[:2], want[:2], ("first", "links")):
        assert len(g) == len(w), (what, name, len(g), len(w))
        if name == "links":
            for f in ("target", "freq", "size"):
                assert np.array_equal(g[f], w[f]), (what, name, f)
        else:
            assert np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64)), (what, name)
    assert {k: int(v) for k, v in got[2].items()} == want[2], (what, got[2], want[2])


def ecoli():
    """capi.Scaffolder on the two E. coli runs: the four files that depend on contig lengths only, and every counter"""
    from dbg_assembly_amd import capi
    res = {}
    for case in LR.golden_cases(CASES):
        if "lengths" not in case:
            continue
        P, names, lens, _, recs, _ = LR.load_case(CASES, case)
        want = LR.expected_outputs(CASES, case)
        with capi.Scaffolder(P.m, P.n, P.i) as s:
            s.set_contigs(lens)
            for r in recs:
                s.add_pairs(r)
            s.build()
            same_table(s.table(), LR.build_table(P, lens, np.concatenate(recs)), case["name"])
            summ = s.resolve()
            pos, rep = s.pos_tabs(names)
            got = {"scaffold.links.all": s.links_text(0), "scaffold.links.uniq": s.links_text(1), "scaffold.pos.tab": pos,
                   "scaffold_repeat.pos.tab": rep}
            ctr = s.table()[2]
            st = s.batch_stats()
        for kind, text in got.items():
            assert text == want[LR.output_name(case, P, kind)], (case["name"], kind)
        c = case["counters"]
        assert {k: int(ctr[k]) for k in LR.COUNTERS} == {k: c[k] for k in LR.COUNTERS}
        assert (summ["lowfreq"], summ["interleave"], summ["repeat_nodes"], summ["deleted"], summ["scaffolds"]) == \
            (c["lowfreq"], c["interleave"], c["repeat"], c["deleted"], c["scaffolds"]), (summ, c)
        res[case["name"]] = {"records": st["records"], "kept": st["kept"], "links": st["links"]}
    assert len(res) == 2
    return res


def hits():
    """add_hits on what capi.Mapper returns for the map_pair fixtures == add_pairs on the parsed 2ctg golden text of the same case"""
    from dbg_assembly_amd import capi
    res = {}
    for case in json.load(open(os.path.join(MAP_CASES, "cases.json"))):
        if case["program"] != "map_pair":
            continue
        MP = MR.params_of(case["args"])
        ids, contigs = MR.read_contig_file(os.path.join(MAP_CASES, case["contigs"]), MP.l)
        index = {name: c for c, name in enumerate(ids)}
        lens = [len(c) for c in contigs]
        files = MR.read_lib_file(os.path.join(MAP_CASES, case["lib"]))
        per_file = []
        with capi.Mapper(k=MP.k, s=MP.s, r=MP.r, identity=MP.i, second_alignment=False) as m:
            m.set_contigs(contigs)
            for f1, f2 in zip(files[0::2], files[1::2]):
                recs = MR.records_map_pair(os.path.join(MAP_CASES, f1), os.path.join(MAP_CASES, f2), MP.fmt)
                h = m.map_sequences([q.encode("latin-1") for r in recs for q in (r[1], r[3])])
                text = gzip.open(os.path.join(MAP_CASES, case["name"], os.path.basename(f1) + ".map_pair.2ctg.gz")).read().decode("latin-1")
                rows = []
                for line in text.split("\n"):
                    if line[:1] == "#" or not line:
                        continue
                    v = LR.split(line)
                    rows.append((index[v[4]], int(v[6]), int(v[7]), index[v[14]], int(v[16]), int(v[17]), ord(v[8]), ord(v[18]), (0, 0)))
                per_file.append((h[0::2], h[1::2], np.array(rows, dtype=LR.PAIR_DTYPE)))
        n_text = sum(len(p[2]) for p in per_file)
        assert n_text > 0
        n_links = []
        for P in (LR.Params(0, 1, 5000), LR.Params(1, 1, 5000), LR.Params(0, 3, 401)):
            tables = []
            for mode in ("hits", "pairs"):
                with capi.Scaffolder(P.m, P.n, P.i) as s:
                    s.set_contigs(lens)
                    for h1, h2, rows in per_file:
                        if mode == "hits":
                            s.add_hits(h1, h2)
                        else:
                            s.add_pairs(rows)
                    s.build()
                    tables.append(s.table())
                    recs_seen = s.batch_stats()["records"]
                assert recs_seen == (sum(len(p[0]) for p in per_file) if mode == "hits" else n_text)
            t = tables[1]
            same_table(tables[0], (t[0], t[1], {k: int(v) for k, v in t[2].items()}), case["name"])
            same_table(tables[1], LR.build_table(P, lens, np.concatenate([p[2] for p in per_file])), case["name"])
            assert sum(tables[0][2].values()) == n_text
            n_links.append(len(tables[0][1]))
        assert max(n_links) > 0                              # (an insert size of 5000 keeps the pairs of these 2 kb contigs)
        res[case["name"]] = {"pairs": sum(len(p[0]) for p in per_file), "two_contig_pairs": n_text, "links": n_links}
    assert len(res) == 3
    return res


def large_records(rng, n_contigs, n):
    lens = rng.integers(200, 5000, n_contigs).astype(np.uint32)
    recs = np.zeros(n, dtype=LR.PAIR_DTYPE)
    c1 = rng.integers(0, n_contigs, n)
    c2 = (c1 + rng.integers(1, 4, n)) % n_contigs
    hot = rng.random(n) < 0.05                             # a twentieth of the records on 40 contig pairs: links far beyond 1023
    c1[hot] = rng.integers(0, 40, int(hot.sum())) * 1000
    c2[hot] = c1[hot] + 1
    recs["contig1"], recs["contig2"] = c1, c2
    for c, s, e in ((c1, "start1", "end1"), (c2, "start2", "end2")):
        recs[s] = (rng.random(n) * lens[c]).astype(np.int32) + 1
        recs[e] = np.minimum(recs[s] + 249, lens[c])
    d = np.frombuffer(b"FFFFRRRRN", dtype=np.uint8)
    recs["direct1"], recs["direct2"] = d[rng.integers(0, 9, n)], d[rng.integers(0, 9, n)]
    d1 = recs["direct1"].copy()
    d1[hot] = ord("F")
    recs["direct1"] = d1
    d2 = recs["direct2"].copy()
    d2[hot] = ord("R")
    recs["direct2"] = d2
    return lens, recs


def large():
    """3 M random records over 100 k contigs in unequal batches (an empty one among them) == the restatement, table and walk"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(11)
    n_contigs, n = 100000, 3000000
    lens, recs = large_records(rng, n_contigs, n)
    P = LR.Params(m=0, n=3, i=3000)
    with capi.Scaffolder(P.m, P.n, P.i) as s:
        s.set_contigs(lens)
        cuts = [0, 1, 1, 777777, 777777 + 1500001, n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            s.add_pairs(recs[a:b])
        s.build()
        got = s.table()
        summ = s.resolve()
        scaf_first, items, repeats = s.layout()
        st = s.batch_stats()
    want = LR.build_table(P, lens, recs)
    same_table(got, want, "large")
    assert int(got[1]["freq"].max()) == 1023 and int((got[1]["freq"] == 1023).sum()) >= 40
    names = ["ctg_%d" % (2 * c + 1) for c in range(n_contigs)]
    res = LR.run(P, names, lens, [recs], ["x"])
    c = res["counters"]
    assert (summ["lowfreq"], summ["interleave"], summ["repeat_nodes"], summ["deleted"], summ["scaffolds"]) == \
        (c["lowfreq"], c["interleave"], c["repeat"], c["deleted"], c["scaffolds"]), (summ, c)
    flat = [(-1 if cc is None else cc, b) for it in res["layout"] for cc, b in it]
    assert items.tolist() == [list(x) for x in flat] or [tuple(x) for x in items.tolist()] == flat
    assert np.array_equal(np.diff(scaf_first.astype(np.int64)), [len(it) for it in res["layout"]])
    return {"records": n, "kept": st["kept"], "links": st["links"], "scaffolds": summ["scaffolds"], "repeat_nodes": summ["repeat_nodes"],
            "ms_orient": st["ms_orient"], "ms_sort": st["ms_sort"], "ms_reduce": st["ms_reduce"], "ms_chain": st["ms_chain"]}


def emit():
    """contigs of 1 base up to more than 2^20, gaps of 1 up to 10^5, every byte value below 128 in a reversed contig"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(3)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNnRYKMSWBDHVryx-*", dtype=np.uint8)
    sizes = [1, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 4097, 65536, (1 << 20) + 3, 300001, 5, 1]
    contigs = [alphabet[rng.integers(0, len(alphabet), n)].tobytes() for n in sizes]
    contigs.append(bytes(range(1, 128)))
    contigs.append(b"")
    items = []
    for _ in range(400):
        if rng.random() < 0.3:
            items.append((-1, int(rng.choice([1, 1, 2, 7, 8, 9, 100, 12345, 100000]))))
        else:
            c = int(rng.integers(0, len(contigs)))
            if len(contigs[c]) > 70000 and rng.random() < 0.7:
                c = int(rng.integers(0, 13))
            items.append((c, int(rng.integers(0, 2))))
    items += [(16, 1), (-1, 100000), (16, 0), (20, 1), (20, 0), (21, 1), (0, 1), (-1, 1)]
    want = LR.emit_string([c.decode("latin-1") for c in contigs], [(None if c < 0 else c, v) for c, v in items]).encode("latin-1")
    with capi.Scaffolder() as s:
        got = s.emit(contigs, np.array(items, dtype=capi.LINK_ITEM_DTYPE)).tobytes()
        one = s.emit(contigs, np.array([(0, 1)], dtype=capi.LINK_ITEM_DTYPE)).tobytes()
        none = s.emit(contigs, np.zeros(0, dtype=capi.LINK_ITEM_DTYPE)).tobytes()
        st = s.batch_stats()
    assert len(got) == len(want) and got == want
    assert one == LR.reverse_complement(contigs[0].decode("latin-1")).encode("latin-1") and none == b""
    return {"bytes": len(want), "items": len(items), "ms_emit": st["ms_emit"]}


if __name__ == "__main__":
    print(json.dumps({"ecoli": ecoli, "hits": hits, "large": large, "emit": emit}[sys.argv[1]]()))
