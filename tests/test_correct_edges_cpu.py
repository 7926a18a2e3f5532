"""CPU: the corrector's edge scenarios (tests/correct_edge_cases.py).  The restatement alone finds what every read was built to
have; on every pinned scenario it equals, byte for byte, what the real reference wrote (tests/golden/correct_edges); one-token
mutants of the restatement change an answer in the category built against them, so the cases discriminate.  No GPU."""
import gzip
import json
import os
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import correct_edge_cases as E  # noqa: E402
import correct_restatement as CR  # noqa: E402

EDGES = os.path.join(ROOT, "tests", "golden", "correct_edges")
REF = os.path.join(ROOT, "oracle", "_ref", "ref_correct")
MAX_FIXTURE_BYTES = 256 << 10
NAMES = [s.name for s in E.scenarios()]
PINNED = [s.name for s in E.scenarios() if s.pinned]


def golden_meta():
    return {c["name"]: c for c in json.load(open(os.path.join(EDGES, "cases.json")))}


def golden_fa(name):
    return gzip.open(os.path.join(EDGES, name + ".correct.fa.gz"), "rb").read()


def by_cat(cat):
    return [(s, e, r) for s in E.scenarios() if s.cat == cat for e, r in zip(s.expect, E.restated(s.name))]


@pytest.mark.parametrize("name", NAMES)
def test_every_read_has_the_properties_it_was_built_for(name):
    s = E.scenario(name)
    assert len(s.reads) == len(s.expect) <= 300 and all(len(r) <= 1100 for r in s.reads)
    for i, (read, e, r) in enumerate(zip(s.reads, s.expect, E.restated(name))):
        assert e["cat"] == s.cat
        for key in ("runs", "one_base", "tree", "deleted", "lt", "rt", "hits", "path", "out", "max_frontier"):
            if key in e:
                assert r[key] == e[key], (name, i, key, e[key], r[key])
        assert r["path"] == (0 if not r["runs"] else 2 if len(read) > 1024 or r["max_frontier"] > 256 else 1)
        if e.get("lt_gt0"):
            assert r["lt"] > 0, (name, i)
        if e.get("rt_gt0"):
            assert r["rt"] > 0, (name, i)
        if "depth0" in e:
            first = r["trees"][0]
            assert first["right"] and not first["modify"] and len(first["frontiers"]) == e["depth0"], (name, i)
        if "zero_word" in e:
            w = e["zero_word"]
            assert not any(r["mask"][64 * w:64 * w + 64]) and any(r["mask"][:64 * w]) and any(r["mask"][64 * w + 64:])
        if "full_word" in e:
            w = e["full_word"]
            assert all(r["mask"][64 * w:64 * w + 64]) and sum(r["mask"]) == 64
        if "low_at" in e:
            assert r["mask"][e["low_at"]] == 0 and CR.seq2bit(read[e["low_at"]:e["low_at"] + s.k]) >= 4 ** s.k
        if "both_ext" in e:
            ext = [t for t in r["trees"] if t["modify"]]
            assert [t["right"] for t in ext] == [False, True] and r["tree"] == 2


def test_every_category_holds_the_shapes_it_lists():
    cats = {c: by_cat(c) for c in E.CATEGORIES}
    assert all(cats[c] for c in E.CATEGORIES)
    k = 13
    mw = [e for _, e, _ in cats["mask_words"]]
    assert {e["nk"] for e in mw if e.get("runs") == []} == set(E.MASK_NKS)
    for which in ("first", "last"):
        assert {e["edge"][1] for e in mw if e.get("edge", ("", 0))[0] == which} == set(E.MASK_EDGES)
    for e in mw:
        if "edge" in e:
            (first, last), = e["runs"]
            assert last - first + 1 == k and (first if e["edge"][0] == "first" else last) == e["edge"][1]
            assert e["one_base"] == 1 and e["path"] == 1 and (e["lt"], e["rt"], e["deleted"]) == (0, 0, 0)
    assert any("inside_word" in e for e in mw) and any("zero_word" in e for e in mw) and any("full_word" in e for e in mw)
    ru = [(s, e, r) for s, e, r in cats["runs"]]
    for c in (0, 2, 3):
        mine = [e for s, e, _ in ru if s.name == "runs_c%d" % c]
        assert {e["two_subs"] for e in mine if "two_subs" in e} == {1, k - 1, k, k + 1}
        assert {e["end_distance"] for e in mine if "end_distance" in e} == {(k - 1, True), (k, False), (150 - k, True), (150 - k - 1, False)}
        assert sum("three" in e for e in mine) == 1 and sum("two_then_one" in e for e in mine) == 1 and sum("short_run" in e for e in mine) == 1
    assert E.scenario("runs_c0").reads == E.scenario("runs_c2").reads == E.scenario("runs_c3").reads
    assert {e["between"] for _, e, _ in ru if "between" in e} == {12, 13, 14} and E.scenario("runs_c4_m").opts["m"] == 13
    assert any(e.get("both_ext") and r["tree"] == 2 for _, e, r in ru)
    assert any(e.get("two_subs") == 1 and r["tree"] == 2 and len(r["trees"]) == 1 for s, e, r in ru if s.name == "runs_c2")   # one tree, two edits
    cl = [e for _, e, _ in cats["classify"]]
    for nk in E.CLASSIFY_NKS:
        assert {e["low_index"] for e in cl if e.get("nk") == nk and "low_index" in e} >= {i for i in (0, 63, 64, 127, 128, nk - 1) if i < nk}
        assert any(e.get("nk") == nk and e["runs"] == [] for e in cl)
    assert {(e["nk"], e["deleted"]) for e in cl if e.get("nk", 99) <= 13} == {(12, 1), (13, 0)}
    assert {e["length"] for e in cl if "length" in e} == {0, k - 1, k}
    assert all((e["path"] == 0) == (e["runs"] == []) for e in cl)
    for kk in (15, 16, 17):
        ob = [e for s, e, _ in cats["one_base_chunks"] if s.k == kk]
        assert E.scenario("one_base_chunks_k%d" % kk).opts == E.opts()
        assert {e["lacks"] for e in ob if "lacks" in e} == {(b, j) for b in "ACGT" for j in range(kk)}
        assert {e["decoy"][1] for e in ob if "decoy" in e} == set(range(kk))
        assert sum("two_pass" in e for e in ob) == 1 and {e["err_byte"] for e in ob if "err_byte" in e} == {"g", "N"}
    assert [(e["length"], e["path"]) for _, e, _ in cats["lds_length"]] == [(1023, 1), (1023, 1), (1024, 1), (1024, 1), (1025, 2), (1025, 2)]
    assert all(e["runs"][0][1] > 1000 for _, e, _ in cats["lds_length"])
    assert [(s.k, s.opts["m"], s.opts["c"], e["max_frontier"], e["path"]) for s, e, _ in cats["frontier_cap"]] == \
        [(kk, M, 1, top, path) for kk in (9, 13) for M, top, path in ((252, 253, 1), (255, 256, 1), (258, 259, 2))]
    assert all(len(s.reads[0]) == 2 * s.opts["m"] + s.k + 40 and s.opts["n"] == E.N_DEFAULT and e["hits"] == 0 for s, e, _ in cats["frontier_cap"])
    n0 = E.node_limit_count()
    assert [(s.opts["n"], e["depth0"], e["hits"]) for s, e, _ in cats["node_limit"]] == [(n0, 39, 3), (n0 + 1, 40, 3)]
    assert all(s.reads == E.scenario("frontier_cap_k9_M255").reads for s, _, _ in cats["node_limit"])
    for x in (5, 17):
        tx = [e for s, e, _ in cats["trim_x"] if s.name == "trim_x%d" % x]
        assert [(e["left_edit"], e["lt"]) for e in tx if "left_edit" in e] == [(x, x), (x + 1, 0)]
        assert [(e["right_edit"], e["rt"]) for e in tx if "right_edit" in e] == [(150 - x + 1, x), (150 - x, 0)]
    (s, e, r), = [t for t in cats["trim_x"] if "clamp" in t[1]]
    assert r["lt"] == len(s.reads[0]) < 24 + s.opts["x"]
    for kk in (1, 2, 3, 4):
        s = E.scenario("small_k%d" % kk + ("_unpinned" if kk == 1 else ""))
        assert s.opts == E.opts(m=3, x=2, r=5) and len(s.reads) == 60 and {len(r) for r in s.reads} == {kk, kk + 1, 30, 64, 65, 100}
        assert 0.4 <= len(s.table.both) / 4 ** kk <= 0.8 and all(s.table.hi(E.rcv(v, kk)) for v in s.table.both)
    s = E.scenario("k19_parity_unpinned")
    lk = cats["large_k"]
    assert s.k == 19 and len(s.reads) == 40 and all(len(r) == 150 for r in s.reads)
    assert sum(r["one_base"] == 1 for _, _, r in lk) >= 10 and sum(r["tree"] == 2 for _, _, r in lk) >= 5
    firsts = {(read[:1], CR.seq2bit(read[:19]) >> 5 > 1 << 32) for read in s.reads if s.table.hi(CR.seq2bit(read[:19]))}
    assert (b"T", True) in firsts and (b"A", False) in firsts
    ob = {s.name: [e["odd"] for e in s.expect] for s, _, _ in cats["odd_bytes"]}
    assert {b for b, _ in ob["odd_bytes_tail"]} == set("X.-R") and all(p >= 150 - k + 1 for _, p in ob["odd_bytes_tail"])
    assert {b for b, _ in ob["odd_bytes_unpinned"]} == set("X.-R") | {128, 200, 255}
    assert not E.scenario("odd_bytes_unpinned").pinned and not s.pinned and not E.scenario("small_k1_unpinned").pinned
    assert [n for n in NAMES if n not in PINNED] == [n for n in NAMES if n.endswith("_unpinned")]


def test_sparse_table_is_the_restatement_table_of_its_raw_file():
    """SparseTable against CR.Table on the bits the loader makes of SparseTable's own raw file, at a k where both fit"""
    from oracle import oracle_py as orc
    import numpy as np
    for name in ("small_k3", "small_k4", "frontier_cap_k9_M255"):
        s = E.scenario(name)
        raw = np.unpackbits(s.table.raw_bytes())
        idx = np.flatnonzero(raw).astype(np.uint64)
        rc = orc.revcomp_values(idx, s.k)
        raw[rc[idx <= rc].astype(np.int64)] = 1
        assert int((idx <= rc).sum()) == s.table.n_canonical()
        T = CR.Table(np.packbits(raw), s.k)
        assert all(T.hi(v) == s.table.hi(v) for v in range(4 ** s.k + 3))
    big = E.scenario("k19_parity_unpinned").table
    blocks = list(big.raw_blocks())
    assert sum(int(np.unpackbits(b).sum()) for _, b in blocks) == big.n_canonical() and all(at % E.BLOCK == 0 and b.any() for at, b in blocks)
    assert not big.hi(4 ** 19) and max(at for at, _ in blocks) > 1 << 32


@pytest.mark.parametrize("name", PINNED)
def test_restatement_equals_the_reference_bytes(name):
    s, meta = E.scenario(name), golden_meta()[name]
    assert meta["k"] == s.k and meta["args"][0:2] == ["-k", str(s.k)] and meta["hifreq"] == s.table.n_canonical()
    o = dict(zip(meta["args"][0::2], meta["args"][1::2]))
    assert {key: int(o["-" + key]) for key in "mcxnr"} == s.opts
    recs = CR.read_records(os.path.join(EDGES, meta["reads"]), 2)
    assert recs == list(zip(E.headers(s), s.reads))
    fa, stat, hits = CR.correct_file(recs, s.table, E.params_of(s))
    assert fa == golden_fa(name)
    assert stat == open(os.path.join(EDGES, name + ".correct.stat")).read()
    assert hits == meta["node_limit_hits"] == sum(e.get("hits", 0) for e in s.expect)
    assert (meta["table"] is not None) == (s.k <= 13)


def test_committed_tables_are_the_scenarios_tables():
    seen = {}
    for s in E.scenarios():
        if s.pinned and s.k <= 13:
            seen.setdefault(s.table_name, s)
            assert seen[s.table_name].table.canon == s.table.canon and seen[s.table_name].table.inverted == s.table.inverted
    for tname, s in seen.items():
        path = os.path.join(EDGES, tname + ".cz")
        lens = [int(v) for v in open(path + ".len").read().split()]
        with open(path, "rb") as f:
            raw = b"".join(zlib.decompress(f.read(n)) for n in lens)
        assert raw == s.table.raw_bytes().tobytes(), tname


def test_fixture_holds_small_data_files_only():
    names = sorted(os.listdir(EDGES))
    assert names and all(n == "cases.json" or n.endswith((".fa.gz", ".correct.stat", ".cz", ".cz.len")) for n in names)
    assert all(os.path.getsize(os.path.join(EDGES, n)) < MAX_FIXTURE_BYTES for n in names)
    assert sorted(golden_meta()) == sorted(PINNED)


def mutant(old, new):
    """correct_one_read of a copy of the restatement with one token changed"""
    src = open(CR.__file__).read()
    assert src.count(old) == 1, old
    ns = {}
    exec(compile(src.replace(old, new), "correct_restatement_mutant", "exec"), ns)
    return ns["correct_one_read"]


def answer(r):
    return tuple(r[key] for key in ("out", "one_base", "tree", "deleted", "lt", "rt", "hits", "max_frontier")) + \
        (len(r["trees"][0]["frontiers"]) if r["trees"] else -1,)


MUTANTS = [
    ("if e - s + 1 != k:", "if e - s + 1 > k:", "runs"),
    ("0 < llast <= P.x", "0 < llast < P.x", "trim_x"),
    ("rlast >= L - P.x + 1", "rlast > L - P.x + 1", "trim_x"),
    ("if new and nodes < P.n:", "if new and nodes <= P.n:", "node_limit"),
    ("if e - s + 1 >= P.m]", "if e - s + 1 > P.m]", "runs"),
    ("for j in range(s - 1, e)):", "for j in range(s - 1, e - 1)):", "one_base_chunks"),
    ("        for b in BASES:", "        for b in BASES[::-1]:", "one_base_chunks"),
]


def changed_by(old, new, cat):
    fn = mutant(old, new)
    return [(s.name, i) for s in E.scenarios() if s.cat == cat
            for i, (read, r) in enumerate(zip(s.reads, E.restated(s.name)))
            if answer(E.restate_read(read, s.table, E.params_of(s), fn)) != answer(r)]


@pytest.mark.parametrize("old,new,cat", MUTANTS, ids=[m[1].strip() for m in MUTANTS])
def test_a_one_token_mutant_of_the_restatement_changes_an_answer(old, new, cat):
    assert changed_by(old, new, cat)


def test_skipping_only_shorter_runs_is_the_one_mutant_no_input_can_tell():
    """`e - s + 1 != k` -> `< k` lets runs LONGER than k try the one-base fix.  The fix checks the windows s .. e of the run as
    they stand; of a run longer than k the first window does not hold the substituted base (it ends k - 1 bases after its start,
    the base lies more than that behind it) and is low by the definition of the run, so the check can never pass: the mutant
    computes what the original does on every input.  The half of `!=` that can be told apart is `> k` (a run of k - 1, in
    MUTANTS above); this test keeps the other half on record on the cases built around k."""
    assert changed_by("if e - s + 1 != k:", "if e - s + 1 < k:", "runs") == []


@pytest.mark.skipif(not os.access(REF, os.X_OK), reason="oracle/_ref/ref_correct not built (no reference sources here)")
def test_live_reference_equals_the_committed_golden(tmp_path):
    s, meta = E.scenario("mask_words"), golden_meta()["mask_words"]
    rfile = tmp_path / "mask_words.fa"
    rfile.write_bytes(E.reads_file(s))
    (tmp_path / "reads.lib").write_text(" %s \n" % rfile)
    subprocess.run([REF] + meta["args"] + [os.path.join(EDGES, meta["table"]), str(tmp_path / "reads.lib")], capture_output=True,
                   check=True, timeout=600)
    assert gzip.open(str(rfile) + ".correct.fa.gz", "rb").read() == golden_fa("mask_words")
    assert open(str(rfile) + ".correct.stat").read() == open(os.path.join(EDGES, "mask_words.correct.stat")).read()
