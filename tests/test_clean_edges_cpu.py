"""CPU: the crafted CLEAN cases of tests/clean_edge_cases.py exercise what they claim -- the restatement alone yields, for every
read, the hit, the tying cells with their lanes and rounds, the block and the break points the read was built to have -- every
category sits on its boundary, the restatement reproduces what the real reference wrote for them (tests/golden/clean_edges),
and every one-token mutant of the lane-by-lane formulation and of the block rule changes the answer of a crafted read."""
import gzip
import json
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_edge_cases as E  # noqa: E402
import clean_restatement as CR  # noqa: E402

EDGES = os.path.join(ROOT, "tests", "golden", "clean_edges")
REFERENCE = os.path.join(os.environ.get("DBGK_REFERENCE", "/root/reference"), "clean_illumina")


def edge_golden_cases():
    return json.load(open(os.path.join(EDGES, "cases.json")))


def every(cat):
    return [(scn, n, e) for scn in E.scenarios() for n, e in enumerate(scn.expect) if e["cat"] == cat]


def only_N(ad):
    return bool(ad) and set(ad) == {"N"}


def crafted_pairs(scn):
    """(read index, adapter index) of every alignment a scenario makes, but for those against a contaminant of N alone, which has
    no positive cell in any formulation (test_formulations_agree_on_a_contaminant_of_N_alone)"""
    for n, h in enumerate(E.restated(scn.name)):
        tried = range(len(scn.adapters)) if h[0] < 0 else range(h[0] + 1)
        for a in tried:
            if scn.reads[n] and scn.adapters[a][1] and not only_N(E.text(scn.adapters[a][1])):
                yield n, a


@pytest.mark.parametrize("name", [s.name for s in E.adapter_scenarios()])
def test_restatement_yields_the_intended_hits_and_four_formulations_agree(name):
    scn = E.scenario(name)
    hits = E.restated(name)                                     # align_many
    adapters = E.named_adapters(scn)
    assert len(scn.reads) == len(scn.expect) == len(hits) > 0
    lanes = {}
    for n, a in crafted_pairs(scn):
        read, ad = E.text(scn.reads[n]), adapters[a][1]
        plain = CR.align(read, ad)
        lanes[n, a] = CR.align_lanes(read, ad)
        assert plain == CR.align_matrix(read, ad) == lanes[n, a]["hit"], (name, n, a)
        assert (plain[0] >= scn.cutoff) == (hits[n][0] == a), (name, n, a)
        if hits[n][0] == a:
            assert hits[n][1:] == plain, (name, n, a)
    for n, (read, e, h) in enumerate(zip(scn.reads, scn.expect, hits)):
        at = (name, n, e)
        assert e["form"] == ("global" if sum(len(s) for _, s in scn.adapters) > E.SET_BYTES or len(read) > E.SLICE else "lds"), at
        if "hit" in e:
            assert tuple(h) == tuple(e["hit"]), (at, h)
        elif "score" in e:
            assert (h[1], (h[2], h[3])) == (e["score"], e["read"]), (at, h)
        else:
            assert e["pad"]                                          # a neighbour of a staged read: nothing is stated of its own hit
        if h[0] < 0:
            continue
        top, cells = CR.max_cells(E.text(read), adapters[h[0]][1])
        assert top == h[1] and cells[0] == (h[3], h[5]), (at, cells)           # the first maximum in row-major order is the hit
        got = lanes[n, h[0]]
        A = len(adapters[h[0]][1])
        assert (got["lane"], got["round"]) == CR.lane_of(h[3], h[5], A), (at, got)
        if "cells" in e:
            assert cells == e["cells"], (at, cells)
        if "lanes" in e:
            assert [CR.lane_of(i, j, A) for i, j in cells] == e["lanes"], at
            # a lane shows the one cell its fold kept: per lane the first of its cells in row-major order
            kept = {}
            for (i, j), (lane, rnd) in zip(cells, e["lanes"]):
                kept.setdefault(lane, (lane, rnd, i, j))
            assert sorted(got["ties"]) == sorted(kept.values()), (at, got)
        if "lane" in e:
            assert (got["lane"], got["round"]) == (e["lane"], e["round"]), (at, got)


def test_formulations_agree_on_a_contaminant_of_N_alone():
    for read in ("T" * 30 + E.text(E.M), "N" * 40, "n"):
        for ad in ("N" * 130, "N"):
            assert CR.align(read, ad) == CR.align_matrix(read, ad) == CR.align_lanes(read, ad)["hit"] == (0, 0, 0, 0, 0)
            assert CR.max_cells(read, ad) == (0, [])


@pytest.mark.parametrize("name", [s.name for s in E.lowqual_scenarios()])
def test_restatement_yields_the_intended_blocks(name):
    scn = E.scenario(name)
    table = CR.error_table(scn.shift)
    assert len(scn.reads) == len(scn.expect) > 0
    for n, ((bases, quals), e, b) in enumerate(zip(scn.reads, scn.expect, E.restated(name))):
        at = (name, n, e)
        breaks = []
        assert CR.lowqual_block(E.text(bases), E.text(quals), scn.cutoff, scn.shift, table, breaks=breaks) == b
        if "block" in e:
            assert tuple(b[1:4]) == tuple(e["block"]), (at, b)
            assert (breaks if b[3] else None) == e["breaks"], (at, breaks)
        else:
            assert bool(b[3]) == e["trimmed"], (at, b)


def test_every_category_sits_on_its_boundary():
    cats = {e["cat"] for scn in E.scenarios() for e in scn.expect}
    assert cats == set(E.CATEGORIES)
    n_ad = sum(len(s.reads) for s in E.adapter_scenarios())
    n_lq = sum(len(s.reads) for s in E.lowqual_scenarios())
    assert 300 <= n_ad <= 3000 and 1500 <= n_lq <= 2800, (n_ad, n_lq)
    assert max(len(r) for s in E.adapter_scenarios() for r in s.reads) == 1100
    # rounds: every (diagonals, adapter length) with a read of at least one base, the winner on every listed diagonal
    seen = {(e["n"], e["A"], e["t"]) for _, _, e in every("rounds")}
    assert seen == {(n, A, t) for n in E.ROUND_N for A in E.ROUND_A if n - A + 1 >= 1 for t in E.round_targets(n)}
    assert {e["n"] for _, _, e in every("rounds")} == set(E.ROUND_N) and {e["A"] for _, _, e in every("rounds")} == set(E.ROUND_A)
    for n in E.ROUND_N:
        lanes = {(e["lane"], e["round"]) for _, _, e in every("rounds") if e["n"] == n}
        assert (0, 0) in lanes and ((n - 1) % 64, (n - 1) // 64) in lanes and ((63, 0) in lanes) == (n >= 64), n
        assert (0, (n - 1) // 64) in lanes                                       # the first lane of the last round
    for scn, n, e in every("rounds"):
        assert scn.cutoff == 1 and e["hit"][1] == 1 and len(scn.reads[n]) + e["A"] - 1 == e["n"]
        assert e["first_diagonal"] == (e["hit"][3] == 1 and e["hit"][5] == e["A"])          # d = -(A - 1)
        assert e["last_diagonal"] == (e["hit"][3] == len(scn.reads[n]) and e["hit"][5] == 1)   # d = L - 1
    assert any(e["first_diagonal"] for _, _, e in every("rounds")) and any(e["last_diagonal"] for _, _, e in every("rounds"))
    # ties: every category through both forms, with what makes it that category
    for cat in E.TIE_CATEGORIES:
        forms = {e["form"] for _, _, e in every(cat)}
        assert forms == {"lds", "global"}, cat
        assert sorted(e["hit"] for _, _, e in every(cat) if e["form"] == "lds") == sorted(e["hit"] for _, _, e in every(cat) if e["form"] == "global")
    for _, _, e in every("tie_same_lane_same_end"):
        (i1, j1), (i2, j2) = e["cells"]
        assert i1 == i2 and j2 - j1 == 64 and e["lanes"][0][0] == e["lanes"][1][0] and e["lanes"][0][1] == e["lanes"][1][1] + 1
    assert {e["lane"] for _, _, e in every("tie_same_lane_same_end")} >= {0, 63}        # the two ends of a round among them
    both = set()
    for _, _, e in every("tie_same_lane_earlier_end"):
        assert len({lane for lane, _ in e["lanes"]}) == 1 and len({i for i, _ in e["cells"]}) == 2
        first_round = min(r for _, r in e["lanes"])
        early = min(i for i, _ in e["cells"])
        both.add(any(i == early and r == first_round for (i, _), (_, r) in zip(e["cells"], e["lanes"])))
        assert e["hit"][3] == early
    assert both == {True, False}                     # the earlier end in the earlier round, and in the later round
    for _, _, e in every("tie_lanes_end"):
        assert len({lane for lane, _ in e["lanes"]}) == len(e["cells"]) == 4 and len({i for i, _ in e["cells"]}) == 2
    for _, _, e in every("tie_lanes_diag"):
        assert len({lane for lane, _ in e["lanes"]}) == 2 and len({i for i, _ in e["cells"]}) == 1
    for _, _, e in every("tie_three"):
        assert len(e["cells"]) == 3 and len({lane for lane, _ in e["lanes"]}) == 2
    assert {e["how"] for _, _, e in every("run_reset")} == {"to_zero", "below_zero", "survives", "twice_two_runs", "twice_one_run"}
    for _, _, e in every("run_reset"):
        if e["how"] in ("to_zero", "below_zero"):
            assert e["hit"][4] > 1                   # the winning run lies behind the reset
    assert {e["how"] for _, _, e in every("overhang")} == {"read_start", "read_end", "adapter_longer", "one_by_one"}
    for scn, n, e in every("overhang"):
        L, A = len(scn.reads[n]), len(scn.adapters[max(e["hit"][0], 0)][1])
        if e["how"] == "read_start":
            assert e["hit"][2] == 1 and e["hit"][4] > 1
        if e["how"] == "read_end":
            assert e["hit"][3] == L and e["hit"][5] < A and e["hit"][4] == 1
        if e["how"] == "adapter_longer":
            assert (L, A) == (20, 130)
        if e["how"] == "one_by_one":
            assert (L, A) == (1, 1)
    # staging: every length at every byte offset mod 4; the batch ends with a read of exactly the slice at offset mod 4 = 3
    stg = E.scenario("staging")
    offs = [0]
    for q in stg.reads:
        offs.append(offs[-1] + len(q))
    for n, e in enumerate(stg.expect):
        assert e["offset_mod4"] == offs[n] % 4 and e["length"] == len(stg.reads[n]) and e["last"] == (n == len(stg.reads) - 1)
        if not e["pad"]:      # the neighbours hold exactly what would extend the match
            k = e["length"] if e["length"] <= 5 else 9
            assert stg.reads[n - 1].endswith(E.M[:5]) and stg.reads[n].startswith(E.M[5:5 + k])
            assert e["last"] or stg.reads[n + 1].startswith(E.M[5 + k:])
            assert e["length"] <= 5 or stg.reads[n].endswith(E.M[:9])
    assert [(e["length"], e["offset_mod4"]) for e in stg.expect if not e["pad"]][-1] == (E.SLICE, 3) and stg.expect[-1]["last"]
    assert sorted((e["length"], e["offset_mod4"]) for e in stg.expect if not e["pad"]) == sorted((L, o) for L in E.STAGED for o in range(4))
    assert E.census(E.scenario("slice_edge")) == {"reads": 3, "by_lds": 1, "by_global": 2}
    assert [len(r) for r in E.scenario("slice_edge").reads] == [1024, 1025, 1100]
    # set sizes: the last contaminant's last bases are the set's last bytes, and the only hit
    assert [sum(len(s) for _, s in E.scenario("set_size_%d" % t).adapters) for t in E.SET_SIZES] == list(E.SET_SIZES)
    for t in E.SET_SIZES:
        scn = E.scenario("set_size_%d" % t)
        c = E.census(scn)
        assert (c["by_lds"], c["by_global"]) == ((3, 0) if t <= E.SET_BYTES else (0, 3))
        last = len(scn.adapters) - 1
        assert scn.adapters[last][1].endswith(E.M) and {e["hit"][0] for e in scn.expect} == {last, -1}
        assert all(e["hit"][5] == len(scn.adapters[last][1]) for e in scn.expect if e["hit"][0] == last)
    for s in E.adapter_scenarios():
        total = sum(len(a) for _, a in s.adapters)
        assert (total > E.SET_BYTES) == (s.fill > 0 or s.name == "set_size_4097"), s.name
    assert {e["how"] for _, _, e in every("order")} == {"first_to_reach", "equal_cutoff", "below_cutoff", "behind_empty", "empty_read", "single_adapter"}
    order = E.scenario("order")
    assert [len(s) for _, s in order.adapters] == [8, 0, 14]
    for n, e in enumerate(order.expect):
        if e["how"] == "first_to_reach":
            assert CR.align(E.text(order.reads[n]), E.text(order.adapters[2][1]))[0] == e["later_score"] > e["hit"][1] == order.cutoff
        if e["how"] == "below_cutoff":
            assert max(CR.align(E.text(order.reads[n]), E.text(s))[0] for _, s in order.adapters) == e["best"] == order.cutoff - 1
        if e["how"] == "behind_empty":
            assert e["hit"][0] == 2
    assert len(E.scenario("tiny").adapters) == 1
    hows = {e["how"] for _, _, e in every("letters")}
    assert hows == {"N_N", "n_N", "base_N", "lower_read", "R_R", "base_R", "other_byte", "lower_adapter", "lower_both", "Y_Y", "y_Y", "high_byte"}
    assert {e["byte"] for _, _, e in every("letters") if e["how"] == "other_byte"} == set(b"-.*")
    assert {e["byte"] for scn, _, e in every("letters") if scn.name == "letters_high_read_unpinned"} == set(E.HIGH_BYTES)
    for scn, n, e in every("letters"):
        if e["how"] == "high_byte" and scn.name == "letters_high_read_unpinned":
            assert e["byte"] in scn.reads[n] and chr(e["byte"] & 0x7F) in "ACGTacgt"
    for size in E.WAVES:
        scn = E.scenario("waves_%d" % size)
        assert len(scn.reads) == size and [e["hit"][0] for e in scn.expect] == [-1] * (size - 1) + [0]
    # lowqual
    for name, (cutoff, Q, top) in E.EQUAL_RATE.items():
        scn = E.scenario(name)
        assert (scn.cutoff, scn.shift) == (cutoff, 33) and [len(b) for b, _ in scn.reads] == list(range(1, top + 1))
        assert all(set(q) == {33 + Q} for _, q in scn.reads) and CR.error_table(33)[33 + Q] == cutoff      # pow(10, -Q / 10) is the cutoff itself
        assert {e["trimmed"] for e in scn.expect} == {True, False}
    cut = {name: [e["length"] for e in E.scenario(name).expect if e["trimmed"]] for name in E.EQUAL_RATE}
    assert cut == {"equal_rate_q30": list(range(10, 21)), "equal_rate_q20": [6] + list(range(18, 31)), "equal_rate_q10": list(range(15, 31))}
    assert {e["how"] for _, _, e in every("breaks")} == {"every_base", "first_only", "last_only", "not_trimmed", "empty"}
    for scn, n, e in every("breaks"):
        L = len(scn.reads[n][0])
        assert e["how"] != "every_base" or (e["breaks"] == list(range(L)) and set(scn.reads[n][1]) == {33 + 2})
        assert e["how"] != "last_only" or (e["breaks"] == [L - 1] and e["block"] == (1, L - 1, 1))
        assert e["how"] != "first_only" or e["breaks"] == [0]
    assert {e["how"] for _, _, e in every("equal_blocks")} == {"two_equal", "three_equal", "later_longer", "tail_equal", "tail_longer"}
    assert {(e["how"], e["shift"]) for _, _, e in every("N")} == {(h, s) for h in "Nn" for s in (33, 64)}
    assert {e["how"] for _, _, e in every("quality_bytes")} == {"table_end", "below_shift", "high", "high_base"}
    qb = E.scenario("quality_bytes_shift20")
    assert qb.shift + 99 == 119 and list(qb.reads[0][1]) == [119] + list(range(120, 128)) + [119] and all(v < qb.shift for v in qb.reads[1][1])
    # chunks: the workgroups begin at offset mod 4 = 0, 1, 2, 3; the break points lie on the two sides of a chunk edge
    ch = E.scenario("chunks")
    offs = [0]
    for b, _ in ch.reads:
        offs.append(offs[-1] + len(b))
    assert len(ch.reads) == 5 * E.GROUP + 3 and [offs[g * E.GROUP] % 4 for g in range(4)] == [0, 1, 2, 3]
    for g in range(4):
        base = offs[g * E.GROUP] & ~3
        own = [(n, ch.expect[n]) for n in range(g * E.GROUP, (g + 1) * E.GROUP)]
        assert all(e.get("wg_first_mod4", g) == g for _, e in own)
        edges = {}
        for n, e in own:
            if e["how"] == "straddle":
                (j,) = e["breaks"]
                edges[e["edge"]] = (offs[n] + j - base) % E.CHUNK
                assert (offs[n] - base) // E.CHUNK < (offs[n + 1] - 1 - base) // E.CHUNK           # the read lies in two chunks
        assert edges == {"last": E.CHUNK - 1, "first": 0}, g
        if g:
            assert ch.reads[own[0][0]] == (b"", b"") and ch.reads[own[-1][0]] == (b"", b"")
    assert sorted(e["length"] for e in ch.expect if e["how"] == "long") == [8192, 8193, 16500]
    assert all(r == (b"", b"") for r in ch.reads[4 * E.GROUP:5 * E.GROUP]) and all(b for b, _ in ch.reads[5 * E.GROUP:])
    for size in E.GROUPS:
        scn = E.scenario("groups_%d" % size)
        assert len(scn.reads) == size
        assert [e["index"] for e in scn.expect if e["telling"]] == ([0] if size == 1 else [n for n in E.TELLING if n < size])


def test_only_what_the_reference_cannot_define_is_unpinned():
    unpinned = [s for s in E.scenarios() if not E.pinned(s)]
    assert sorted(s.name for s in unpinned) == ["letters_high_adapter_unpinned", "letters_high_read_unpinned", "quality_bytes_high_unpinned"]
    assert {e["cat"] for s in unpinned for e in s.expect} == E.UNPINNED_CATEGORIES
    for s in unpinned:          # each holds a byte from 128 on, which indexes outside the reference's alphabet[128] / Qual2Err[128]
        blob = b"".join(s.reads) + b"".join(a for _, a in s.adapters) if isinstance(s, E.AdapterScenario) else b"".join(b + q for b, q in s.reads)
        assert max(blob) >= 128
    for s in E.scenarios():
        if E.pinned(s):
            blob = b"".join(s.reads) + b"".join(a for _, a in s.adapters) if isinstance(s, E.AdapterScenario) else b"".join(b + q for b, q in s.reads)
            assert not blob or max(blob) < 128, s.name
    assert sorted(c["name"] for c in edge_golden_cases()) == sorted(s.name for s in E.scenarios() if E.pinned(s))


def test_golden_set_is_the_generators():
    """the committed inputs of tests/golden/clean_edges are what the generator builds today"""
    for case in edge_golden_cases():
        scn = E.scenario(case["name"])
        assert case == E.case_of(scn)
        assert gzip.open(os.path.join(EDGES, case["input"]), "rb").read() == E.fastq(scn)
        recs = CR.load_reads(os.path.join(EDGES, case["input"]))
        if isinstance(scn, E.AdapterScenario):
            assert open(os.path.join(EDGES, scn.name + ".fa"), "rb").read() == E.fasta(scn)
            assert CR.case_adapters(EDGES, case) == E.named_adapters(scn)
            assert [s.encode("latin-1") for _, s, _ in recs] == list(scn.reads)
        else:
            assert [(s.encode("latin-1"), q.encode("latin-1")) for _, s, q in recs] == list(scn.reads)


@pytest.mark.parametrize("case", edge_golden_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_edge_golden(case):
    """what the real programs wrote for the pinned scenarios; the numbers are the ones every other test here uses"""
    want = CR.expected_outputs(EDGES, case)
    numbers = E.restated(case["name"])
    got = CR.run_case(EDGES, case, hits=numbers, blocks=numbers)
    assert got["out"] == want["out"]
    assert got["stat"] == want["stat"]


def changed_by(mutant, cats):
    out = []
    for scn in E.adapter_scenarios():
        if scn.fill:
            continue
        for n, e in enumerate(scn.expect):
            h = E.restated(scn.name)[n]
            if e["cat"] in cats and h[0] >= 0:
                read, ad = E.text(scn.reads[n]), E.text(scn.adapters[h[0]][1])
                if CR.align_lanes(read, ad, mutant)["hit"] != h[1:]:
                    out.append((scn.name, n, e["cat"]))
    return out


ADAPTER_MUTANT_FOUND_BY = {
    "reset_lt": {"run_reset"}, "first_ge": {"tie_same_lane_earlier_end", "run_reset"}, "fold_no_tie": {"tie_same_lane_same_end"},
    "fold_re_gt": {"tie_same_lane_earlier_end"}, "fold_d_lt": {"tie_same_lane_same_end"}, "reduce_max_end": {"tie_lanes_end"},
    "reduce_min_diag": {"tie_lanes_diag", "tie_lanes_end"}, "mask_5f": {"letters"}}


@pytest.mark.parametrize("mutant", sorted(ADAPTER_MUTANT_FOUND_BY))
def test_adapter_mutant_changes_a_crafted_read(mutant):
    found = {c for _, _, c in changed_by(mutant, set(E.ADAPTER_CATEGORIES))}
    assert found >= ADAPTER_MUTANT_FOUND_BY[mutant], (mutant, found)


def test_the_guard_below_128_is_implied_by_the_mask():
    """Dropping `c < 128` from clean_code changes nothing on any input: `c & 0xDF` keeps bit 7, so a byte from 128 on never
    equals 0x41, 0x43, 0x47 or 0x54 behind the mask -- the mutant is equivalent, and no read can tell.  Its other half is what
    the guard stands for: the six bytes that equal a letter in their low seven bits code as 4 like every other byte from 128
    on, which the mask that would fold bit 7 away (mutant mask_5f) gets wrong and the crafted reads notice."""
    assert set(CR.ALIGN_MUTANTS) == set(ADAPTER_MUTANT_FOUND_BY) | {"no_128_guard"}
    for c in range(256):
        assert CR.lane_code(c) == CR.lane_code(c, "no_128_guard") == CR.CODE.get(chr(c) if c < 128 else "", 4), c
    assert not changed_by("no_128_guard", {"letters"})
    for c in E.HIGH_BYTES:
        assert CR.lane_code(c) == 4 and CR.lane_code(c, "mask_5f") < 4
    found = changed_by("mask_5f", {"letters"})
    assert {E.scenario(s).expect[n]["byte"] for s, n, _ in found if s == "letters_high_read_unpinned"} == set(E.HIGH_BYTES)
    assert any(s == "letters_high_adapter_unpinned" for s, _, _ in found)


LOWQUAL_MUTANT_FOUND_BY = {"break_ge": "equal_rate", "longest_ge": "equal_blocks", "tail_ge": "equal_blocks", "N_keeps_quality": "N",
                           "n_counts_as_N": "N", "pairwise_sum": "equal_rate"}


@pytest.mark.parametrize("mutant", sorted(LOWQUAL_MUTANT_FOUND_BY))
def test_lowqual_mutant_changes_a_crafted_block(mutant):
    assert set(LOWQUAL_MUTANT_FOUND_BY) == set(CR.LOWQUAL_MUTANTS)
    found = set()
    for scn in E.lowqual_scenarios():
        if scn.name == "chunks" or scn.name.startswith("groups"):
            continue
        table = CR.error_table(scn.shift)
        for (bases, quals), e, b in zip(scn.reads, scn.expect, E.restated(scn.name)):
            got = CR.lowqual_block(E.text(bases), E.text(quals), scn.cutoff, scn.shift, table, mutant=mutant)
            if struct.pack("<d3i", *got) != struct.pack("<d3i", *b):
                found.add(e["cat"])
    assert LOWQUAL_MUTANT_FOUND_BY[mutant] in found, (mutant, found)
    if mutant == "pairwise_sum":     # another order of summation flips the decision itself, not only the last bit of the sum
        flips = 0
        for name in E.EQUAL_RATE:
            scn = E.scenario(name)
            for (bases, quals), b in zip(scn.reads, E.restated(name)):
                flips += CR.lowqual_block(E.text(bases), E.text(quals), scn.cutoff, scn.shift, mutant=mutant)[3] != b[3]
        assert flips > 0


@pytest.mark.parametrize("case", edge_golden_cases(), ids=lambda c: c["name"])
def test_reference_programs_still_write_the_goldens(tmp_path, case):
    """live: where the reference's ready-built programs are at hand, they write today what tests/golden/clean_edges holds"""
    exe = os.path.join(REFERENCE, case["program"])
    if not os.access(exe, os.X_OK):
        pytest.skip("the reference's %s is not on this machine" % case["program"])
    r = subprocess.run([exe] + case["args"] + [case["input"], str(tmp_path / "out.gz"), str(tmp_path / "out.stat")], cwd=EDGES,
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = CR.expected_outputs(EDGES, case)
    assert gzip.decompress((tmp_path / "out.gz").read_bytes()).decode("latin-1") == want["out"]
    assert (tmp_path / "out.stat").read_bytes().decode("latin-1") == want["stat"]
