"""CPU: the LINK / FILL edge scenarios of tests/scaffold_edge_cases.py sit where they claim.  From the restatements alone: every
scenario has the properties its `expect` names; the naive record-by-record restatements agree with the vectorised ones on every
scenario; and both reproduce what the real reference wrote for the subset stored in tests/golden/scaffold_edges."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fill_restatement as FR  # noqa: E402
import link_restatement as LR  # noqa: E402
import scaffold_edge_cases as E  # noqa: E402

EDGES = os.path.join(ROOT, "tests", "golden", "scaffold_edges")


def golden_cases():
    return json.load(open(os.path.join(EDGES, "cases.json")))


def fill(name):
    return next(f for f in E.fill_scenarios() if f.name == name)


def link(name):
    return next(s for s in E.link_scenarios() if s.name == name)


def same_table(a, b, what):
    assert np.array_equal(np.asarray(a[0], dtype=np.int64), np.asarray(b[0], dtype=np.int64)), (what, "first")
    for f in ("target", "freq", "size"):
        assert np.array_equal(a[1][f], b[1][f]), (what, f)
    assert dict(a[2]) == dict(b[2]), (what, a[2], b[2])


def spanning(f, res, pair):
    """the records of a pair's mode in file order, and their slices as the restatement cuts them"""
    mode, _, _, _, span = res["stats"][pair]
    return mode, span, [f.reads[int(f.recs[r]["read"])][int(f.recs[r]["align1_end"]):][:mode] for r in span.tolist()]


# ---- FILL -------------------------------------------------------------------------------------------------------------------

def test_widths_x_spans_fills_every_width_at_every_span():
    f = fill("widths_x_spans")
    res = E.fill_result(f.name)
    gaps = E.filled_gaps(res)
    assert len(f.recs) == 5312 and f.cuts == [0, 1, 1, 5312 // 3, 5312]
    assert sorted((g[1], g[2]) for g in gaps) == f.expect["filled"] and len(gaps) == 64
    assert any(float(g[6]) < 1 for g in gaps) and any(float(g[6]) == 1 for g in gaps)
    assert max(g[1] for g in gaps) == 200 and max(g[2] for g in gaps) == 200          # four units, four rounds of reads
    exact = 0
    for pair, (mode, mf, tf, var, span) in res["stats"].items():
        r = f.recs[span]
        assert set(r["direct1"].tolist()) == ({ord("F"), ord("R")} if mf > 1 else {ord("F")})   # both strands in every gap
        room = r["read_len"] - r["align1_end"] - mode
        assert room.min() == 0 and room.max() <= 2                                    # a slice that ends with its read
        exact += int((room == 0).sum())
        assert tf == mf + (2 if mf > 2 else 0)
        runs = sorted(set(FR.gaps_of(f.recs[(np.minimum(f.recs["contig1"], f.recs["contig2"]) == pair[0])]).tolist()))
        if mf > 2:
            assert runs.index(mode) == (0 if mode == 1 else 1)                        # the mode is not the only run of its pair
    assert exact >= 64
    assert sorted(set(f.recs["read"].tolist())) == list(range(len(f.recs)))


def test_column_ties_hold_every_tied_pair_and_the_widest_tie():
    f = fill("column_ties")
    res = E.fill_result(f.name)
    cons = {(g[1], g[2]): g for g in E.filled_gaps(res)}
    assert sorted(cons) == [(130, 10), (130, 12)]
    for pair, x in f.expect["gaps"].items():
        mode, span, slices = spanning(f, res, pair)
        assert mode == 130 and len(span) == x["span"]
        rows = [FR.rev_com_seq(s) if f.recs[r]["direct1"] == ord("R") else s for s, r in zip(slices, span.tolist())]
        assert sum(f.recs[r]["direct1"] == ord("R") for r in span.tolist()) == x["span"] // 2
        counts = [tuple(sum(row[k] == ch for row in rows) for ch in E.LETTERS) for k in range(130)]
        assert counts == x["counts"]                                                  # the columns hold what they were dealt
        got, freqs, _ = FR.consensus(rows)
        assert got == x["consensus"] == cons[(130, x["span"])][5] and freqs == [max(c) for c in counts]
        tied = {tuple(i for i in range(5) if c[i] == max(c)) for c in counts}
        assert {t for t in tied if len(t) == 2} == {(i, j) for i in range(5) for j in range(i + 1, 5)}   # A=C ... N=T
        widest = 5 if x["span"] % 5 == 0 else 4
        for k in E.TIE_COLUMNS:
            assert sum(v == max(counts[k]) for v in counts[k]) == widest, k
        if widest == 4:                                                               # each letter absent in turn: A A A A C wins
            assert [x["consensus"][k] for k in E.TIE_COLUMNS[:5]] == ["C", "A", "A", "A", "A"]
        else:
            assert all(x["consensus"][k] == "A" for k in E.TIE_COLUMNS)
    assert sorted(len(x["counts"]) for x in f.expect["gaps"].values()) == [130, 130]


def test_host_path_late_places_its_odd_bytes():
    f = fill("host_path_late")
    res = E.fill_result(f.name)
    odd = []
    for g, pair in enumerate(f.expect["pairs"]):
        mode, span, slices = spanning(f, res, pair)
        assert mode == 129 and len(span) == 70
        where = [(m, k, s[k]) for m, s in enumerate(slices) for k in range(129) if s[k] not in "ACGTN"]
        odd.append(where)
        if g == 2:
            assert not where and any("N" in s for s in slices)
    assert odd[0] == [(69, 128, "g")] and f.recs[res["stats"][f.expect["pairs"][0]][4][69]]["direct1"] == ord("F")
    assert len(odd[1]) == 35 and {(k, c) for _, k, c in odd[1]} == {(128, "\xc1")} and odd[1][-1][0] == 69
    by_pair = []
    for its in res["layout"]:
        ctg = [it[1] for it in its if it[0] == "ctg"]
        by_pair += [(tuple(sorted(ctg[k:k + 2])), it) for k, it in enumerate(x for x in its if x[0] == "gap")]
    by_pair = dict(by_pair)
    a, b, c = (by_pair[p] for p in f.expect["pairs"])
    assert a[5][128] in "ACGT" and np.float32(a[6]) < 1 and b[5][128] == "\xc1" and "N" not in c[5]
    assert f.expect["host_path"] == [1, 1, 0]


@pytest.mark.parametrize("name", ["gapstat_runs", "gapstat_last_single"])
def test_gapstat_runs_sit_on_the_gallop_edges(name):
    f = fill(name)
    res = E.fill_result(name)
    assert {k: v[:4] for k, v in res["stats"].items()} == f.expect["stats"] == E.naive_gap_stats(f.recs)
    g = FR.gaps_of(f.recs)
    assert g.min() >= -40 and g.max() <= 60 and f.n == 1
    lengths, where = set(), set()
    for pair, spec in f.expect["runs"].items():
        assert [x[0] for x in spec] == sorted(x[0] for x in spec)
        mode, mf = res["stats"][pair][:2]
        lengths |= {c for _, c in spec}
        top = [k for k, (_, c) in enumerate(spec) if c == mf]
        assert spec[top[0]][0] == mode                                                # on a tie the smallest gap
        if len(spec) == 3:
            where.add(top[0])
    assert lengths >= set(E.RUN_LENGTHS) and where == {0, 1, 2}                       # the mode first, in the middle, last
    first, last = min(f.expect["runs"]), max(f.expect["runs"])
    assert first == (0, 1) and last == (len(f.lens) - 2, len(f.lens) - 1)             # sorted position 0, and the run that ends at n
    assert res["stats"][last][:2] == ((17, 1) if name == "gapstat_last_single" else (21, 1025))
    cut, mixed = f.expect["cut"], f.expect["mixed"]
    assert res["stats"][cut][:3] == (-3, 4, 8)                                        # {-3 x 4, 2 x 4}: the negative gap is the mode ...
    items = next(its for its in res["layout"] if any(it[0] == "ctg" and it[1] == cut[0] for it in its))
    assert items[0] == ("ctg", cut[0], 0, f.lens[cut[0]] - 3) and items[1][:2] == ("gap", -3)   # ... and cuts the left contig by 3
    r = f.recs[(np.minimum(f.recs["contig1"], f.recs["contig2"]) == mixed[0])]
    assert (r["contig1"] < r["contig2"]).sum() == 4 and (r["contig1"] > r["contig2"]).sum() == 3 and (r["direct2"] == ord("N")).sum() == 1
    assert res["stats"][mixed][:3] == (12, 4, 7)                                      # pooled into one statistic
    ties = [spec for spec in f.expect["runs"].values() if sorted(c for _, c in spec)[-2:] in ([3, 3], [4, 4], [6, 6])]
    assert len(ties) >= 4 and any(len({c for _, c in spec}) == 1 and len(spec) == 3 for spec in ties)   # two-way and three-way


def test_slice_jobs_sit_on_the_end_of_the_read():
    jobs = E.slice_jobs()
    assert [j.name for j in jobs] == ["exact"] + [k % at for at in E.BAD_AT for k in ("short_%d", "negative_%d")] + ["modes_not_positive"]
    for j in jobs:
        f = j.fill
        if j.refused:
            with pytest.raises(ValueError):
                E.run_fill(f)
            at = int(j.name.split("_")[1])
            base = jobs[0].fill
            diff = [k for k in range(len(f.recs)) if f.recs[k] != base.recs[k] or f.reads[k] != base.reads[k]]
            assert diff == [at]                                                       # one read, at the spanning index named
            r = f.recs[at]
            if j.name.startswith("short"):
                assert int(r["align1_end"]) + 70 == len(f.reads[at]) + 1              # one byte longer than its read
            else:
                assert int(r["align1_end"]) == -1 and int(FR.gaps_of(f.recs[at:at + 1])[0]) == 70
        else:
            res = E.run_fill(f)
            assert len(E.filled_gaps(res)) == j.filled
            if j.name == "exact":
                for pair, (mode, mf, _, _, span) in res["stats"].items():
                    r = f.recs[span]
                    assert np.array_equal(r["align1_end"] + mode, [len(f.reads[k]) for k in r["read"].tolist()])   # ends exactly
                assert sorted(v[1] for v in res["stats"].values()) == [3, 130]
            else:
                assert all(v[0] <= 0 for v in res["stats"].values()) and max(len(x) for x in f.reads) == 5
                assert (f.recs["align1_end"] > 5).all()


def test_more_units_than_waves_is_one_unit_per_junction():
    f = fill("more_units_than_waves")
    res = E.fill_result(f.name)
    gaps = E.filled_gaps(res)
    assert len(gaps) == E.UNITS_JUNCTIONS == 40000 and all(g[2] == 3 and 1 <= g[1] <= 3 for g in gaps)
    assert sum((g[1] + 63) // 64 for g in gaps) == 40000 > 16 * 4 * 256              # more units than an MI355X's 256 CUs take at once


def test_fill_hits_hold_every_drop_condition():
    h = E.fill_hits()
    n = len(h.lens)
    assert set(h.kinds) == set(E.HIT_KINDS) and h.first_reads == [0, 7] and h.hits.shape == (len(h.kinds), 2)
    c1, c2 = h.hits["contig"][:, 0], h.hits["contig"][:, 1]
    for kind, cond in (("hit1_unmapped", c1 == -1), ("hit2_unmapped", c2 == -1), ("same_contig", c1 == c2), ("contig_is_n", (c1 == n) | (c2 == n)),
                       ("contig_minus_2", (c1 == -2) | (c2 == -2))):
        assert [k for k, x in zip(h.kinds, cond.tolist()) if x] == [kind] * 4, kind
    plain = (c1 != -1) & (c2 != -1) & (c1 != c2) & (c1 >= 0) & (c1 < n) & (c2 >= 0) & (c2 < n)
    assert np.array_equal(h.kept_rows["read"], np.nonzero(plain)[0]) and h.expect["kept"] == 20 == int(plain.sum())
    for f, col, which in (("align1_end", "read_end", 0), ("align2_start", "read_start", 1), ("contig1", "contig", 0), ("contig2", "contig", 1),
                          ("direct1", "direct", 0), ("direct2", "direct", 1)):
        assert np.array_equal(h.kept_rows[f], h.hits[col][plain, which]), f
    names = ["ctg_%d" % (2 * c + 1) for c in range(n)]
    res = FR.run(FR.Params(n=1), names, h.lens, [h.kept_rows], ["x"], None, h.reads)
    assert sorted(g[1] for g in E.filled_gaps(res)) == h.expect["modes"] and res["counters"]["wrong"] == 4
    assert min(res["counters"][k] for k in ("FF", "RR", "FR", "RF")) == 4


# ---- LINK -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", E.link_scenarios(), ids=lambda s: s.name)
def test_naive_and_vectorised_link_tables_agree(s):
    same_table(E.naive_link_table(s.P, s.lens, s.recs), LR.build_table(s.P, s.lens, s.recs), s.name)


@pytest.mark.parametrize("m", [0, 1])
def test_naive_and_vectorised_link_tables_agree_on_the_hits(m):
    h = E.link_hits(m)
    same_table(E.naive_link_table(h.P, h.lens, h.kept_rows), LR.build_table(h.P, h.lens, h.kept_rows), h.name)


@pytest.mark.parametrize("m,I", E.FILTER_JOBS)
def test_filter_edges_keep_the_middle_two(m, I):
    s = link("filter_edges_m%d_i%d" % (m, I))
    a_src, a_tgt, b_src, b_tgt, gap, keep, ctr = LR.orient(s.P, s.lens, s.recs)
    assert gap.tolist() == E.gap_edges(I) * 4 and keep.tolist() == [False, True, True, False] * 4
    assert ctr == dict(FR=4, RF=4, FF=4, RR=4, wrong=0)                               # the class counters count all four
    if I == 1:
        assert gap[keep].tolist() == [1] * 8
    first, links, _ = LR.build_table(s.P, s.lens, s.recs)
    assert len(links) == 8 and (links["freq"] == 2).all() and (links["size"] == s.expect["size"]).all()
    for cls, (a, b) in s.expect["pairs"].items():
        rows = s.recs[(s.recs["contig1"] == a)]                                       # each quadruple on a contig pair of its own
        assert len(rows) == 4 and (rows["contig2"] == b).all() and (rows["direct1"] == ord(cls[0])).all() and (rows["direct2"] == ord(cls[1])).all()


def test_cap_runs_straddle_a_batch_cut_and_the_large_insert_sum_passes_2_31():
    s = link("cap_across_batches")
    x = s.expect
    first, links, _ = LR.build_table(s.P, s.lens, s.recs)
    assert len(s.cuts) == 6 and x["cut"] in s.cuts
    for k, c in enumerate(x["counts"]):
        at = np.nonzero(x["key_of"] == k)[0]
        assert len(at) == c
        if c > LR.FREQ_CAP:
            assert at[LR.FREQ_CAP - 1] < x["cut"] <= at[LR.FREQ_CAP]                  # record 1023 | record 1024 of every key
        assert np.any(np.diff(at) > 1)                                                # dealt between records of other keys
    got = {}
    for k, c in enumerate(x["counts"]):
        row = links[int(first[4 * k + 1]):int(first[4 * k + 2])]                      # contig 2k forward -> contig 2k + 1 forward
        assert len(row) == 1 and row["target"][0] == 4 * k + 3
        got[k] = (int(row["freq"][0]), int(row["size"][0]))
    assert [got[k] for k in range(5)] == [(min(c, 1023), x["sizes"][k]) for k, c in enumerate(E.CAP_COUNTS)]
    assert [x["sizes"][k] for k in range(5)] == [-7154, -7161, -7161, -7161, -7161]   # one record more or less shows in the sum
    assert got[x["big_key"]] == (1023, x["big_size"]) and x["big_size"] > 2 ** 31 and s.P.i == E.BIG_INSERT
    # at the cap: both directed entries of the keys of 1023, 1024, 1025 and 2047 records and of the large-insert key, nothing else
    assert int((links["freq"] == 1023).sum()) == 2 * 5 and int(links["freq"].max()) == 1023 and got[0][0] == 1022
    gap = LR.orient(s.P, s.lens, s.recs)[4]
    assert np.abs(gap).max() < 2 ** 31 - 1 and LR.orient(s.P, s.lens, s.recs)[5].all()


def test_first_seen_order_is_neither_sorted_order():
    s = link("first_seen_order")
    first, links, _ = LR.build_table(s.P, s.lens, s.recs)
    a = links["target"][int(first[1]):int(first[2])].tolist()
    b = links["target"][int(first[3]):int(first[4])].tolist()
    assert a == s.expect["first"] == sorted(a, reverse=True) and len(a) == 200
    assert b == s.expect["second"] and b != sorted(b) and b != sorted(b, reverse=True) and len(b) == 40
    assert (links["freq"][int(first[1]):int(first[2])] == 2).all()                    # the second sighting moved nothing
    src = np.repeat(np.arange(len(first) - 1), np.diff(first))
    into = np.bincount(links["target"], minlength=len(first))
    assert into.max() <= 255 and np.diff(first).max() == 200                          # inside the reference's 8-bit counters
    assert int(into[2]) == 200 and sum(1 for t in a if len(links[int(first[t + 1]):int(first[t + 2])]) == 1) == 200 - len(b)
    of_0 = (s.recs["contig1"] == 0) | (s.recs["contig2"] == 0)
    seen = [int(np.nonzero(of_0 & ((s.recs["contig2"] == (t - 1) // 2) | (s.recs["contig1"] == (t - 1) // 2)))[0][0]) for t in a]
    assert seen == sorted(seen) and seen[0] < s.cuts[1] <= seen[80] and seen[100] < s.cuts[2] <= seen[-1] and len(src) == len(links)


@pytest.mark.parametrize("m", [0, 1])
def test_link_hits_hold_every_drop_condition(m):
    h = E.link_hits(m)
    n = len(h.lens)
    c1, c2 = h.hits1["contig"], h.hits2["contig"]
    assert set(h.kinds) == set(E.HIT_KINDS)
    plain = (c1 != -1) & (c2 != -1) & (c1 != c2) & (c1 >= 0) & (c1 < n) & (c2 >= 0) & (c2 < n)
    assert int(plain.sum()) == len(h.kept_rows) == 20
    for f, col, hh in (("contig1", "contig", h.hits1), ("start1", "contig_start", h.hits1), ("end1", "contig_end", h.hits1),
                       ("contig2", "contig", h.hits2), ("start2", "contig_start", h.hits2), ("end2", "contig_end", h.hits2),
                       ("direct1", "direct", h.hits1), ("direct2", "direct", h.hits2)):
        assert np.array_equal(h.kept_rows[f], hh[col][plain]), f
    first, links, ctr = LR.build_table(h.P, h.lens, h.kept_rows)
    assert ctr == dict(FR=4, RF=4, FF=4, RR=4, wrong=4) and len(links) > 0
    assert (h.kept_rows["contig1"] != h.kept_rows["contig2"]).all()                   # nothing map_pair would not write


# ---- the stored reference output ----------------------------------------------------------------------------------------------

def test_goldens_are_the_subset_and_hold_no_program_text():
    cases = golden_cases()
    assert [c["name"] for c in cases] == [f.name for f in E.fill_golden_scenarios()] + [s.name for s in E.link_scenarios()]
    for case in cases:
        assert os.path.getsize(os.path.join(EDGES, case["name"] + ".zip")) <= 200 * 1024
        assert all(not n.endswith((".cpp", ".h", ".py", ".pl", ".sh")) and "Makefile" not in n for n in LR.case_files(EDGES, case))


@pytest.mark.parametrize("case", [c for c in golden_cases() if c["program"] == "link_contig"], ids=lambda c: c["name"])
def test_fill_restatements_reproduce_the_reference(case):
    f = next(x for x in E.fill_golden_scenarios() if x.name == case["name"])
    P, names, seqs, recs, files, reads = FR.load_case(EDGES, case)
    assert P.n == f.n and [len(q) for q in seqs] == list(f.lens) and reads == list(f.reads)
    assert np.array_equal(np.concatenate(recs), f.recs)                               # the stored input IS the scenario
    want = LR.expected_outputs(EDGES, case)
    got, res = FR.run_case(EDGES, case)
    assert len(want) == 7
    FR.compare_outputs(case, got, want)
    assert {k: v[:4] for k, v in res["stats"].items()} == E.naive_gap_stats(f.recs)
    gaps = E.filled_gaps(res)
    if f.name == "widths_x_spans_cut":
        assert sorted((g[1], g[2]) for g in gaps) == f.expect["filled"] and len(gaps) == 15
    elif f.name == "column_ties":
        assert sorted(g[5] for g in gaps) == sorted(x["consensus"] for x in f.expect["gaps"].values())
    elif f.name == "host_path_late":
        assert sum("\xc1" in g[5] for g in gaps) == 1 and "\xc1" in want["res_host_path_late.contig_R.seq.fa"]
    else:
        assert max(v[1] for v in res["stats"].values()) == 1024 and res["stats"][f.expect["cut"]][0] == -3


@pytest.mark.parametrize("case", [c for c in golden_cases() if c["program"] == "link_scaffold"], ids=lambda c: c["name"])
def test_link_restatements_reproduce_the_reference(case):
    s = link(case["name"])
    P, names, lens, seqs, recs, files = LR.load_case(EDGES, case)
    assert P == s.P and list(lens) == list(s.lens) and [len(r) for r in recs] == np.diff(s.cuts).tolist()
    assert np.array_equal(np.concatenate(recs), s.recs)                               # the stored input IS the scenario
    want = LR.expected_outputs(EDGES, case)
    got, res = LR.run_case(EDGES, case)
    assert sorted(got) == sorted(want) and len(want) == (5 if "lengths" in case else 7)
    for f in want:
        assert got[f] == want[f], (case["name"], f)
    same_table(E.naive_link_table(s.P, s.lens, s.recs), LR.build_table(s.P, s.lens, s.recs), s.name)
    if s.name == "cap_across_batches":                                                # a sum beyond 2^31 in the reference's own text
        assert "\t%d,1023,%d,%d" % (4 * 5 + 3, s.expect["big_size"], s.expect["big_size"] // 1023) in want[LR.output_name(case, P, "scaffold.links.all")]
