"""CPU: the crafted map cases of tests/map_edge_cases.py exercise what they claim -- the restatement alone yields, for every
read, the seed window, direction, extension lengths, mismatch count, acceptance and second hit the read was built to have --
and the restatement reproduces what the real reference wrote for them (tests/golden/map_edge_cases)."""
import gzip
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_edge_cases as E  # noqa: E402
import map_restatement as MR  # noqa: E402

EDGE_CASES = os.path.join(ROOT, "tests", "golden", "map_edge_cases")


def edge_golden_cases():
    return json.load(open(os.path.join(EDGE_CASES, "cases.json")))


def edge_expected(case):
    """{output file name: text} of what the reference wrote for a case of the edge set"""
    return json.loads(gzip.open(os.path.join(EDGE_CASES, case["name"] + ".out.json.gz")).read())


def every(cat):
    return [(scn, n, e) for scn in E.scenarios() for n, e in enumerate(scn.expect) if e["cat"] == cat]


@pytest.mark.parametrize("name", [q.name for q in E.scenarios()])
def test_restatement_yields_the_intended_properties(name):
    scn = next(q for q in E.scenarios() if q.name == name)
    X, hits = E.restated(name)
    P = E.params_of(scn)
    k, s = scn.k, scn.s
    assert len(scn.reads) == len(scn.expect) == len(hits)
    for n, (read, e, (h1, h2)) in enumerate(zip(scn.reads, scn.expect, hits)):
        at = (name, n, e)
        if e.get("skipped"):
            assert len(read) < max(scn.r, k + s) and (h1, h2) == (MR.NO_HIT, MR.NO_HIT), at
            continue
        seed = MR.get_align_seed(X, read, 1, P)
        assert seed is not None and seed[3] == e["seed"] + 1, (at, seed)              # the window that seeds
        assert seed[0] == e["contig"] and chr(h1.direct) == seed[5] == e["direct"], (at, seed)
        assert h1.align_len == k + s + e["left"] + e["right"], (at, h1)
        assert h1.mismatches == e["mis"], (at, h1)
        assert (h1.contig != -1) == e["accepted"] and h1.contig in (-1, e["contig"]), (at, h1)
        if "hit" in e:
            assert tuple(h1) == e["hit"], (at, h1)
        elif e["direct"] == "F":      # the aligned stretch in the contig's orientation
            assert h1.read_start == e["seed"] + 1 - e["left"] and h1.read_end == e["seed"] + k + s + e["right"], (at, h1)
        else:
            assert h1.read_start == e["seed"] + 1 - e["right"] and h1.read_end == e["seed"] + k + s + e["left"], (at, h1)
        assert h1.contig_end - h1.contig_start == h1.read_end - h1.read_start or "hit" in e, (at, h1)
        if e["second"] == "none":
            assert h2 == MR.NO_HIT, (at, h2)
        elif e["second"] == "hit":
            assert scn.second and h2.contig not in (-1, h1.contig) and h2.read_start > h1.read_end, (at, h2)
        else:
            assert scn.second and h2.contig == -1 and h2.align_len >= k + s, (at, h2)


def test_every_category_sits_on_its_boundary():
    cats = {e["cat"] for scn in E.scenarios() for e in scn.expect}
    assert cats == set(E.CATEGORIES)
    assert {(q.k, q.s) for q in E.scenarios()} == set(E.PARAMS)
    total = sum(len(q.reads) for q in E.scenarios())
    assert 300 <= total <= 1500, total
    # ramp: every first window c - 1, c, c + 63, c + 64, c + 127, c + 128 of the first chunks 1, 4 and 64, F and R, per (k, s)
    for k, s in E.GOLDEN_PARAMS:
        seen = {(e["first_window"], e["direct"]) for scn, n, e in every("ramp") if (scn.k, scn.s) == (k, s)}
        assert seen == {(c + d, f) for c in E.RAMPS for d in (-1, 0, 63, 64, 127, 128) for f in "FR"}
        assert all(e["seed"] == e["first_window"] == e["left" if e["direct"] == "F" else "right"] for scn, n, e in every("ramp"))
        # both extension loops at every length, ended by the read and by the contig, in both directions
        for cat, limit in (("ext_read_end", "read"), ("ext_contig_end", "contig")):
            got = {(e["ext"], e["direct"]) for scn, n, e in every(cat) if (scn.k, scn.s) == (k, s)}
            assert got == {((side, n), f) for side in ("left", "right") for n in E.EXT_LENGTHS for f in "FR"}
            for scn, n, e in every(cat):
                side, length = e["ext"]
                assert e[side] == length and e["limit"] == limit
                hang = len(scn.reads[n]) - (scn.k + scn.s + e["left"] + e["right"])          # read bases beyond the contig's end
                assert hang == (5 if limit == "contig" else 0)
    for scn, n, e in every("ext_mismatch_stride2"):
        assert e["mis"] == 2 and e["seed"] == 0 and e["left" if e["direct"] == "R" else "right"] == 129
    for scn, n, e in every("ext_mismatch_last"):
        assert e["mis"] == 1 and e["seed"] == 0 and e["left" if e["direct"] == "R" else "right"] == e["ext"]
    assert {(e["ext"], e["limit"], e["direct"]) for _, _, e in every("ext_mismatch_last")} >= {
        (n, "read", f) for n in (1, 63, 64, 65, 129) for f in "FR"} | {(n, "contig", f) for n in (64, 129) for f in "FR"}
    assert {(e["flush"], e["direct"]) for _, _, e in every("flush")} == {(w, f) for w in ("start", "end") for f in "FR"}
    for scn, n, e in every("flush"):
        assert e["left" if e["flush"] == "start" else "right"] == 0 and e["right" if e["flush"] == "start" else "left"] == 6
    for cat in ("partner_missing", "partner_dup", "partner_other_contig"):
        assert all(e["seed"] > 0 for _, _, e in every(cat)), cat
    assert {e["direct"] for _, _, e in every("inverted")} == {"F", "R"}
    for scn, n, e in every("inverted"):
        assert scn.k > scn.s and e["hit"][4] - e["hit"][3] + 1 == scn.k - scn.s
    # staging: every length at every byte offset mod 4 in both directions, seeding in the last window; the batch ends with a
    # read of exactly the slice
    stg = next(q for q in E.scenarios() if q.name == "staging")
    offs = [0]
    for q in stg.reads:
        offs.append(offs[-1] + len(q))
    for n, e in enumerate(stg.expect):
        assert e["offset_mod4"] == offs[n] % 4
        if e["cat"] == "staging":
            assert e["seed"] == len(stg.reads[n]) - stg.k - stg.s == e["length"] - stg.k - stg.s and e["accepted"]
    assert {(e["length"], e["offset_mod4"], e["direct"]) for e in stg.expect if e["cat"] == "staging"} >= {
        (L, o, f) for L in E.STAGED for o in range(4) for f in "FR"}
    assert [len(q) for q in stg.reads[:4]] == [0, 1, 2, 3] and len(stg.reads[-1]) == E.SLICE and stg.expect[-1]["last"]
    c = E.census(stg)
    assert c["by_long"] == 16 and c["by_lds"] == 17 and c["skipped"] == len(stg.reads) - 33
    # identity: the largest accepted count and one more, for the three thresholds; 9 in 300 is the float case
    assert E.most_accepted(300, 0.97) == 9 and E.most_accepted(299, 0.97) == 8 and E.most_accepted(333, 0.97) == 9
    for name in ("identity_097", "identity_09", "identity_1"):
        scn = next(q for q in E.scenarios() if q.name == name)
        pairs = {}
        for e in scn.expect:
            pairs.setdefault(e["partner"], []).append(e)
        flips = [p for p in pairs.values() if len(p) == 2]
        assert len(flips) >= 5 and {e["direct"] for p in flips for e in p} == {"F", "R"}
        for a, b in flips:
            A = scn.k + scn.s + a["left"] + a["right"]
            assert a["accepted"] and not b["accepted"] and b["mis"] == a["mis"] + 1 == E.most_accepted(A, scn.identity) + 1
    grow = next(q for q in E.scenarios() if q.name == "accept_growth")
    b0, b1 = E.batches(grow)
    assert max(len(grow.reads[n]) for n in b0) <= 200 and {len(grow.reads[n]) for n in b1} == {E.SLICE + 1}
    assert all(grow.expect[n]["left"] + grow.expect[n]["right"] + 36 == E.SLICE + 1 for n in b1)
    assert [grow.expect[n]["accepted"] for n in b1] == [True, True, True, False]
    # second alignment: the gate at k + s - 1 / k + s, a rejected first hit, a rejected second hit, and the same reads without
    on, off = (next(q for q in E.scenarios() if q.name == n) for n in ("second_on", "second_off"))
    assert on.reads == off.reads and on.second and not off.second
    assert {(e["rest"], e["second"]) for e in on.expect if e["cat"] == "second_gate"} == {(35, "none"), (36, "hit"), (80, "hit")}
    assert [(e["accepted"], e["second"]) for e in on.expect if e["cat"] == "second_first_rejected"] == [(False, "none")]
    assert [(e["accepted"], e["second"]) for e in on.expect if e["cat"] == "second_rejected"] == [(True, "rejected")]
    assert all(e["second"] == "none" for e in off.expect)
    # lengths and letters
    for k, s in E.GOLDEN_PARAMS:
        own = [(scn, n, e) for scn, n, e in every("length_edge") if (scn.k, scn.s) == (k, s)]
        assert sorted(len(scn.reads[n]) - k - s for scn, n, e in own) == [-1, -1, 0, 0, 1, 1]
        assert all(bool(e.get("skipped")) == (len(scn.reads[n]) < k + s) for scn, n, e in own)
    for scn, n, e in every("below_r"):
        assert scn.r > scn.k + scn.s and bool(e.get("skipped")) == (len(scn.reads[n]) == scn.r - 1) and len(scn.reads[n]) in (scn.r - 1, scn.r)
    assert all(scn.reads[n] == b"" for scn, n, e in every("empty"))
    for k, s in E.GOLDEN_PARAMS:      # an empty read with a mapped one on either side
        assert any((scn.k, scn.s) == (k, s) and not scn.expect[n - 1].get("skipped") and not scn.expect[n + 1].get("skipped")
                   for scn, n, e in every("empty") if 0 < n < len(scn.reads) - 1)
    for scn, n, e in every("lower_case"):     # bytes are compared: lower case differs from the contig, its complement does not
        assert scn.reads[n].islower() and e["mis"] == (e["right"] if e["direct"] == "F" else 0) and e["left" if e["direct"] == "F" else "right"] == 0
    assert sorted((e["inside"], e["mis"]) for scn, n, e in every("N") if scn.k == 21) == [(False, 1)] * 2 + [(True, 0)] * 2
    for scn, n, e in every("key0"):
        w = scn.reads[n][:scn.k]
        assert w in (b"A" * scn.k, b"T" * scn.k) and MR.window_key(scn.reads[n], 0, scn.k)[0] == 0 and e["seed"] == 0
    for k, s in E.GOLDEN_PARAMS:
        for cats, odd in ((("other_first", "other_last", "other_ext"), b"-R"), (("high_bytes",), b"\x80\xff")):
            own = [(scn, n, e) for c in cats for scn, n, e in every(c) if (scn.k, scn.s) == (k, s)]
            assert {(e["byte"], e["direct"]) for _, _, e in own} == {(b, f) for b in odd for f in "FR"}
            assert all(sum(c in odd for c in scn.reads[n]) == 1 for scn, n, e in own)
    for scn, n, e in every("other_first"):
        assert scn.reads[n][0] == e["byte"] and (e["seed"], e["mis"]) == ((0, 0) if e["found"] else (1, 1))
    for scn, n, e in every("other_last"):
        assert scn.reads[n][scn.k - 1] == e["byte"] and (e["seed"], e["mis"]) == ((0, 0) if e["found"] else (scn.k, 1))
    for scn, n, e in every("other_ext"):
        assert scn.reads[n][scn.k + scn.s + 3] == e["byte"] and (e["seed"], e["mis"]) == (0, 1)
    scn, idx = E.grid_reads(4 * 32 * 256 + 5)
    assert len(set(idx)) == 12 and all(not scn.expect[n].get("skipped") for n in idx)


def test_golden_set_is_the_generators():
    """the committed inputs of tests/golden/map_edge_cases are what the generator builds today"""
    cases = edge_golden_cases()
    want = E.golden_scenarios()
    assert sorted({c["scenario"] for c in cases}) == sorted(q.name for q in want)
    assert {(q.k, q.s) for q in want} == set(E.GOLDEN_PARAMS)
    for scn in want:
        progs = {c["program"]: c for c in cases if c["scenario"] == scn.name}
        assert sorted(progs) == ["map_pair", "map_reads"]
        P = MR.params_of(progs["map_reads"]["args"])
        assert (P.k, P.s, P.r, P.i, P.fmt) == (scn.k, scn.s, scn.r, scn.identity, 2)
        ids, contigs = MR.read_contig_file(os.path.join(EDGE_CASES, progs["map_reads"]["contigs"]), P.l)
        assert [q.encode() for q in contigs] == list(scn.contigs)
        f = MR.read_lib_file(os.path.join(EDGE_CASES, progs["map_reads"]["lib"]))[0]
        got = [r.encode("latin-1") for _, r in MR.records_map_reads(os.path.join(EDGE_CASES, f), 2)]
        assert got == list(scn.reads)


@pytest.mark.parametrize("case", edge_golden_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_edge_golden(case):
    want = edge_expected(case)
    got = MR.run_case(EDGE_CASES, case)
    assert sorted(got) == sorted(want)
    for f in sorted(want):
        assert got[f] == want[f], f
