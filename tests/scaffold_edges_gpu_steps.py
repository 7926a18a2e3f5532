"""GPU steps of tests/test_scaffold_edges_gpu.py, each run in a child process of its own under a time limit:
    python tests/scaffold_edges_gpu_steps.py fill_consensus | fill_gapstat | fill_slices | fill_stride | fill_hits | link_edges | cli_edges
The scenarios are those of tests/scaffold_edge_cases.py; FILL is compared through check_against of tests/fill_gpu_steps.py (table,
gap statistics, layout, consensus bytes, identity as float bits), LINK through same_table of tests/link_gpu_steps.py against the
vectorised and the naive restatement.  Prints one JSON line of findings; exits non-zero on a mismatch.  Times are reported, never
asserted."""
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
import scaffold_edge_cases as E  # noqa: E402
from fill_gpu_steps import check_against  # noqa: E402
from link_gpu_steps import same_table  # noqa: E402

EDGES = os.path.join(ROOT, "tests", "golden", "scaffold_edges")
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")


def filler(f):
    """a built capi.GapFiller over a Fill scenario, its records fed in the scenario's batches"""
    from dbg_assembly_amd import capi
    g = capi.GapFiller(f.n)
    g.set_contigs(f.lens)
    g.set_reads([r.encode("latin-1") for r in f.reads])
    for a, b in zip(f.cuts[:-1], f.cuts[1:]):
        g.add_records(f.recs[a:b])
    g.build()
    return g


def gaps_by_pair(g):
    """{(contig_lo, contig_hi): FILL_GAP_DTYPE row} over the layout"""
    _, items, gaps, _, _ = g.layout()
    out = {}
    items = items.tolist()
    for k, (c, rev, length, gi, off) in enumerate(items):
        if c < 0:
            a, b = items[k - 1][0], items[k + 1][0]
            out[(min(a, b), max(a, b))] = gaps[gi]
    return out


def fill_scenario(f, res=None):
    """a Fill scenario on the device == the restatement -> summary, gaps taken by the host path, the layout's gaps by pair, timing
    (with the gap statistics as st["gap_stats"])"""
    res = res or E.fill_result(f.name)
    with filler(f) as g:
        summ, host_path = check_against(g, res, f.lens, None, f.name)
        by_pair = gaps_by_pair(g)
        st = dict(g.timing(), gap_stats=g.gap_stats())
    assert summ["filled"] == len(E.filled_gaps(res)), (f.name, summ)
    return summ, host_path, by_pair, st


def fill_consensus():
    """FILL 1 to 3: every width at every span, every column tie, the odd byte in the last unit of the last round"""
    by_name = {f.name: f for f in E.fill_scenarios()}
    out = {}
    summ, host_path, by_pair, st = fill_scenario(by_name["widths_x_spans"])
    got = sorted((int(G["mode"]), int(G["mode_freq"])) for G in by_pair.values())
    assert got == by_name["widths_x_spans"].expect["filled"] and host_path == 0, got
    out["widths_x_spans"] = {"filled": summ["filled"], "below_1": sum(float(G["identity"]) < 1 for G in by_pair.values()),
                             "records": st["records"], "ms_consensus": st["ms_consensus"]}
    f = by_name["column_ties"]
    summ, host_path, by_pair, st = fill_scenario(f)
    assert host_path == 0 and sorted(by_pair) == sorted(f.expect["gaps"])          # (check_against compared the bytes column by column)
    out["column_ties"] = {"filled": summ["filled"], "columns": summ["cons_bytes"]}
    f = by_name["host_path_late"]
    summ, host_path, by_pair, st = fill_scenario(f)
    out["host_path_late"] = {"filled": summ["filled"], "host_path": [int(by_pair[p]["host_path"]) for p in f.expect["pairs"]]}
    assert out["host_path_late"]["host_path"] == f.expect["host_path"], out
    return out


def fill_gapstat():
    """FILL 4: runs around the powers of two, position 0, a run that ends at n, sign order, the mode first / in the middle / last"""
    out = {}
    for f in E.fill_scenarios():
        if not f.name.startswith("gapstat"):
            continue
        summ, host_path, by_pair, st = fill_scenario(f)
        rows = st["gap_stats"]
        got = {(int(r["contig_lo"]), int(r["contig_hi"])): tuple(int(r[k]) for k in ("mode", "mode_freq", "total_freq", "variance")) for r in rows}
        assert got == f.expect["stats"], f.name                                # the plain loop of the case file
        out[f.name] = {"pairs": len(rows), "filled": summ["filled"], "max_span": max(v[1] for v in got.values()), "ms_gapstat": st["ms_gapstat"]}
    assert len(out) == 2
    return out


def fill_slices():
    """FILL 5: a slice that ends with its read is legal, one byte more or align1_end = -1 is refused whichever lane group meets
    it, and a gap whose mode is <= 0 never looks at its reads"""
    from dbg_assembly_amd import capi
    refused, resolved = [], {}
    for j in E.slice_jobs():
        if j.refused:
            with filler(j.fill) as g:
                try:
                    g.resolve()
                except capi.DbgkError as e:
                    assert e.status == capi.ERR_ARG, (j.name, e.status)
                    refused.append(j.name)
                else:
                    raise AssertionError("%s: a slice outside its read was accepted" % j.name)
        else:
            summ, host_path, _, _ = fill_scenario(j.fill, E.run_fill(j.fill))
            assert summ["filled"] == j.filled, (j.name, summ)
            resolved[j.name] = summ["filled"]
    return {"refused": refused, "resolved": resolved}


def fill_stride():
    """FILL 6: more work units than the consensus launch has waves"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    f = next(f for f in E.fill_scenarios() if f.name == "more_units_than_waves")
    assert f.expect["units"] > 16 * 4 * cus, "the case must grow: %d units against %d waves" % (f.expect["units"], 16 * 4 * cus)
    summ, host_path, _, st = fill_scenario(f)
    assert summ["filled"] == f.expect["units"] and summ["cons_bytes"] == int(f.expect["widths"].sum())
    return {"units": f.expect["units"], "waves": 16 * 4 * cus, "filled": summ["filled"], "ms_consensus": st["ms_consensus"]}


def fill_hits():
    """FILL 7: add_hits over a hand-made hit array == add_records on the rows a plain filter keeps == the restatement"""
    from dbg_assembly_amd import capi
    h = E.fill_hits()
    names = ["ctg_%d" % (2 * c + 1) for c in range(len(h.lens))]
    res = FR.run(FR.Params(n=1), names, h.lens, [h.kept_rows], ["x"], None, h.reads)
    hits = np.ascontiguousarray(h.hits.astype(capi.MAP_HIT_DTYPE))
    got = []
    for mode in ("hits", "records"):
        with capi.GapFiller(1) as g:
            g.set_contigs(h.lens)
            g.set_reads([q.encode("latin-1") for q in h.reads])
            if mode == "hits":
                cut = h.first_reads[1]
                g.add_hits(hits[:cut], h.first_reads[0])
                g.add_hits(hits[cut:], cut)
            else:
                g.add_records(h.kept_rows)
            g.build()
            t = g.table()
            stats = g.gap_stats().tolist()
            check_against(g, res, h.lens, None, "fill_hits " + mode)
            got.append((t, stats, [x.tolist() for x in g.layout()], g.resolve(), g.timing()))
    same_table(got[0][0], (got[1][0][0], got[1][0][1], {k: int(v) for k, v in got[1][0][2].items()}), "fill_hits")
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2] and got[0][3] == got[1][3]
    assert got[0][4]["records"] == len(h.reads) and got[1][4]["records"] == len(h.kept_rows) and got[0][4]["pooled"] == len(h.kept_rows)
    return {"reads": len(h.reads), "pooled": got[0][4]["pooled"], "filled": got[0][3]["filled"]}


def link_edges():
    """LINK 1 to 4: the table of every scenario == the vectorised and the naive restatement; add_hits == add_pairs of the kept rows"""
    from dbg_assembly_amd import capi
    out = {}
    for s in E.link_scenarios():
        with capi.Scaffolder(s.P.m, s.P.n, s.P.i) as sc:
            sc.set_contigs(s.lens)
            for a, b in zip(s.cuts[:-1], s.cuts[1:]):
                sc.add_pairs(s.recs[a:b])
            sc.build()
            got = sc.table()
            st = sc.batch_stats()
        same_table(got, LR.build_table(s.P, s.lens, s.recs), s.name)
        same_table(got, E.naive_link_table(s.P, s.lens, s.recs), s.name + " (naive)")
        freq = got[1]["freq"]
        out[s.name] = {"records": st["records"], "kept": st["kept"], "links": len(freq), "max_freq": int(freq.max()),
                       "at_cap": int((freq == LR.FREQ_CAP).sum()), "max_size": int(got[1]["size"].max())}
    for m in (0, 1):
        h = E.link_hits(m)
        h1, h2 = (np.ascontiguousarray(x.astype(capi.MAP_HIT_DTYPE)) for x in (h.hits1, h.hits2))
        tables = []
        for mode in ("hits", "pairs"):
            with capi.Scaffolder(h.P.m, h.P.n, h.P.i) as sc:
                sc.set_contigs(h.lens)
                if mode == "hits":
                    for a, b in zip(h.cuts[:-1], h.cuts[1:]):
                        sc.add_hits(h1[a:b], h2[a:b])
                else:
                    sc.add_pairs(h.kept_rows)
                sc.build()
                tables.append(sc.table())
                seen = sc.batch_stats()["records"]
            assert seen == (len(h1) if mode == "hits" else len(h.kept_rows))
        want = LR.build_table(h.P, h.lens, h.kept_rows)
        same_table(tables[0], want, h.name + " hits")
        same_table(tables[1], want, h.name + " pairs")
        assert sum(int(v) for v in tables[0][2].values()) == len(h.kept_rows)
        out[h.name] = {"pairs": len(h1), "kept": len(h.kept_rows), "links": len(tables[0][1])}
    return out


def cli_edges():
    """bin/link_contig and bin/link_scaffold over the golden subset: every file the reference wrote, byte for byte"""
    done = {}
    for case in json.load(open(os.path.join(EDGES, "cases.json"))):
        with tempfile.TemporaryDirectory() as work:
            LR.unpack_inputs(EDGES, case, work)
            if "lengths" in case:                                                   # placeholder sequences of the stored lengths
                with open(os.path.join(work, "contigs.fa"), "w") as fa:
                    for line in open(os.path.join(work, case["lengths"])):
                        name, n = line.split()
                        fa.write(">%s\n%s\n" % (name, "A" * int(n)))
            contigs = case.get("contigs", "contigs.fa")
            r = subprocess.run([os.path.join(BIN, case["program"])] + case["args"] + ["-o", case["prefix"], contigs, case["lib"]], cwd=work,
                               capture_output=True, timeout=240)
            assert r.returncode == 0, (case["name"], r.stderr[-3000:])
            want = LR.expected_outputs(EDGES, case)
            assert len(want) == (5 if "lengths" in case else 7), case["name"]
            for f, text in want.items():
                got = LR.strip_run_time(r.stderr.decode("latin-1")) if f == "stderr.txt" else open(os.path.join(work, f), encoding="latin-1", newline="").read()
                assert got == text, (case["name"], f)
        done[case["name"]] = len(want)
    return done


if __name__ == "__main__":
    steps = {"fill_consensus": fill_consensus, "fill_gapstat": fill_gapstat, "fill_slices": fill_slices, "fill_stride": fill_stride,
             "fill_hits": fill_hits, "link_edges": link_edges, "cli_edges": cli_edges}
    print(json.dumps(steps[sys.argv[1]]()))
