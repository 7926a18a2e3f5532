"""GPU steps of tests/test_simplify_gpu.py, each run in a child process of its own under a time limit:
    python tests/simplify_gpu_steps.py trace | branches | update | counts  narrow | wide31 | above32
Hand-built tables of a few hundred slots go through capi.ContigBuilder.trace / trace_branches / update and every field is compared
with the restatement's get_linear_path (tests/contig_restatement.py:linear_path; above k = 32 on tests/wide_contig_restatement.py's
table, PARITY UNPINNED there).  Mode wide31 runs the 128-bit kernels at k <= 31 on {0, kmer} tables: they must give what the 64-bit
handle gives.  Prints one JSON line of findings; exits non-zero on a mismatch."""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
import wide_contig_restatement as W  # noqa: E402
from contig_gpu_steps import build_table, rand_seq  # noqa: E402

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = str.maketrans("ACGT", "TGCA")
TRACED, BELOW, ABSENT, NOT_LINEAR = 0, 1, 2, 3


def arrays_for(t, wide):
    """the table as ContigBuilder(wide=wide).set_table takes it; a table of 64-bit keys becomes {0, kmer} nodes for a wide handle"""
    from dbg_assembly_amd import capi
    if isinstance(t, W.WideTable) or not wide:
        return t.arrays()
    a, nul, dele, kl = t.arrays()
    w = np.zeros(t.size, dtype=capi.NODE32_DTYPE)
    w["kmer_lo"], w["l_link"], w["r_link"] = a["kmer"], a["l_link"], a["r_link"]
    return w, nul, dele, kl


def make(k, seqs, size):
    t = W.build_table(seqs, k, size) if k > 31 else build_table(seqs, k, size)
    R.first_pass(t, R.Options())
    return t


def key_of(t, s):
    return R.canonical(t, sum(CODE[c] << (2 * (t.k - 1 - j)) for j, c in enumerate(s)))


def flips_on_steps(t):
    out = []
    for u in range(t.size):
        if t.filled[u] and t.linear[u]:
            for d in (1, -1):
                out.append(R.canonical(t, R.next_kmer(t, t.kmer[u], t.r_base[u] if d == 1 else t.l_base[u], d))[1])
    return out


def tables(k, rng):
    """name -> (table, cutoffs): what the trace must get right, at this k"""
    out = {}
    # ten linear nodes between two dead ends: cutoffs around the place where the walk from the first linear node meets the end
    # (9: stops on a linear node exactly at the cutoff; 8 and 10 either side; 0 and 1: one step)
    out["chain10"] = (make(k, [(rand_seq(rng, 10 + k + 1), 5)], 211), (0, 1, 2, 8, 9, 10, 11, 100))
    out["chains"] = (make(k, [(rand_seq(rng, n + k + 1), 5) for n in (1, 2, 3, 5, 30, 64)], 1009), (7, 100))
    t = make(k, [(rand_seq(rng, 40 + k + 1, "AC"), 5)], 211)            # no step flips
    assert not any(flips_on_steps(t))
    out["no_flip"] = (t, (100,))
    if k % 2:                                                            # every step flips (k odd)
        t = make(k, [("".join(rng.choice("AC" if p % 2 == 0 else "GT") for p in range(40 + k + 1)), 5)], 211)
        assert all(flips_on_steps(t))
        out["every_flip"] = (t, (100,))
    else:                                                                # a palindromic k-mer as a linear node on a path (k even)
        half = rand_seq(rng, k // 2)
        pal = half + half.translate(COMP)[::-1]
        t = make(k, [(rand_seq(rng, 30) + pal + rand_seq(rng, 30), 5)], 211)
        pkey, flipped = key_of(t, pal)
        assert flipped and R.revcomp(pkey, k) == pkey and t.linear[t.exist(pkey)]
        out["palindrome"] = (t, (100,))
    # the key-0 node on a path, and as its own neighbour on both sides (a cycle of one node)
    t = make(k, [(rand_seq(rng, 20) + "C" + "A" * k + "C" + rand_seq(rng, 20), 5)], 211)
    assert t.linear[t.exist(0)]
    out["key0"] = (t, (100,))
    out["poly_a"] = (make(k, [("A" * (k + 6), 5), (rand_seq(rng, 30), 5)], 211), (1, 5))
    # a cycle of n linear nodes, shorter than the cutoff of 100: the same slots repeat in nodes
    n = 30 if k < 30 else k + 7
    s = rand_seq(rng, n)
    t = make(k, [(s + s[:k], 5)], 211)
    assert sum(t.linear) == n
    out["cycle"] = (t, (n - 1, n, n + 1, 100))
    # last a branch node: three sequences share a stem; and last absent: the end nodes deleted (a deleted match is absent), one link
    # rewritten to lead to a k-mer that is in no slot
    stem = rand_seq(rng, k + 12)
    t = make(k, [(stem + b + rand_seq(rng, 15), 5) for b in "ACG"], 307)
    assert any(t.r_num[i] == 3 or t.l_num[i] == 3 for i in range(t.size))
    out["fork"] = (t, (100,))
    t = make(k, [(rand_seq(rng, 20 + k + 1), 5), (rand_seq(rng, 20 + k + 1), 5)], 307)
    ends = [i for i in range(t.size) if t.filled[i] and not t.linear[i] and t.kmer[i]]
    for i in ends[:2]:
        t.deleted[i] = True
    lin = [i for i in range(t.size) if t.linear[i]]
    u = lin[len(lin) // 2]
    other = next(b for b in range(4) if b != t.r_base[u] and t.exist(R.canonical(t, R.next_kmer(t, t.kmer[u], b, 1))[0]) == t.size)
    t.r_link[u], t.r_base[u] = 5 << ((3 - other) * 8), other
    t.deleted[lin[3]] = True                                              # a deleted node in the middle of a chain, and a deleted start
    out["absent"] = (t, (100,))
    # a table so full that probe chains wrap past its last slot
    t = make(k, [(rand_seq(rng, 60 + k + 1), 5) for _ in range(3)], 197)
    assert t.filled[0] and t.filled[t.size - 1]
    out["wrap"] = (t, (100,))
    return out


def home(t, s):
    return (W.hash128 if isinstance(t, W.WideTable) else R.hash_code)(t.kmer[s]) % t.size


def probes_that_wrap(t, want):
    """how many nodes that the walks of `want` find by a probe (every node after the start, and last) lie below their home slot: the
    probe that finds one runs past the last slot of the table and on from slot 0"""
    found = {v for w in want for v in w["nodes"][1:] + [w["last"]] if v != t.size}
    return sum(1 for v in found if home(t, v) > v)


def expect_walk(t, s, d, cutoff):
    n, depth, nodes, text, last, mark = R.linear_path(t, s, d, cutoff)
    return dict(start=s, direct=d, status=TRACED, len=n, depth=depth, last=last, mark=1 if mark == "branch" else 0, nodes=nodes, text=text)


def expect_branch_row(t, o, idx, side, j, cutoff):
    direct = 1 if side == 0 else -1
    none = dict(start=t.size, direct=0, len=0, depth=0, last=t.size, mark=0, nodes=[], text="")
    if R.depth_of(t.r_link[idx] if direct == 1 else t.l_link[idx], j) <= o.D:
        return dict(none, status=BELOW)
    key, flipped = R.canonical(t, R.next_kmer(t, t.kmer[idx], j, direct))
    v, d1 = t.exist(key), -direct if flipped else direct
    if v == t.size:
        return dict(none, status=ABSENT, direct=d1)
    if not t.linear[v]:
        return dict(none, status=NOT_LINEAR, start=v, direct=d1)
    return expect_walk(t, v, d1, cutoff)


def compare(got, want, what):
    rows, first, nodes, bases, summ = got
    assert len(rows) == len(want) == summ["rows"], (what, len(rows), len(want), summ)
    assert int(first[0]) == 0 and int(first[-1]) == len(nodes) == len(bases) == summ["nodes"] == sum(w["len"] for w in want), (what, summ)
    assert summ["traced"] == sum(1 for w in want if w["len"]), (what, summ)
    for i, w in enumerate(want):
        r = rows[i]
        g = {f: int(r[f]) for f in ("start", "direct", "status", "len", "depth", "last", "mark")}
        assert g == {f: w[f] for f in g}, (what, i, g, w)
        lo, hi = int(first[i]), int(first[i + 1])
        assert hi - lo == w["len"] and nodes[lo:hi].tolist() == w["nodes"], (what, i, "nodes")
        assert "".join("ACGT"[b] for b in bases[lo:hi]) == w["text"], (what, i, "bases")


def every_request(t):
    """every filled slot both ways: linear or not, deleted or not"""
    return [(s, d) for s in range(t.size) if t.filled[s] for d in (1, -1)]


def handles(t, mode):
    """-> the builders to run: the narrow one, and / or the wide one"""
    from dbg_assembly_amd import capi
    out = []
    for wide in {"narrow": (False,), "wide31": (False, True), "above32": (True,)}[mode]:
        g = capi.ContigBuilder(t.k, wide=wide)
        g.set_table(*arrays_for(t, wide))
        out.append(g)
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def ks_of(mode):
    return (33, 47, 63) if mode == "above32" else (21, 20, 31)


def step_trace(mode):
    out = {}
    for k in ks_of(mode):
        rng = random.Random(100 + k)
        for name, (t, cutoffs) in tables(k, rng).items():
            reqs = every_request(t)
            gs = handles(t, mode)
            for cutoff in cutoffs:
                want = [expect_walk(t, s, d, cutoff) for s, d in reqs]
                assert name != "wrap" or probes_that_wrap(t, want) > 0, (k, "no probe of a walk wraps past the end of the table")
                got = [g.trace([s for s, _ in reqs], [d for _, d in reqs], cutoff) for g in gs]
                compare(got[-1], want, (k, name, cutoff))
                assert len(got) == 1 or same(got[0], got[1]), (k, name, cutoff, "the wide handle differs from the narrow one")
                key = "k%d_%s" % (k, name)
                o = out.setdefault(key, {"requests": 0, "absent": 0, "absent_from_linear": 0, "branch": 0, "cut": 0, "repeats": 0, "max_len": 0})
                o["requests"] += len(want)
                o["absent"] += sum(1 for w in want if w["last"] == t.size)
                o["absent_from_linear"] += sum(1 for w in want if w["last"] == t.size and t.linear[w["start"]])
                o["branch"] += sum(1 for w in want if w["mark"])
                o["cut"] += sum(1 for w in want if w["last"] != t.size and t.linear[w["last"]])
                o["repeats"] += sum(1 for w in want if len(set(w["nodes"])) < len(w["nodes"]))
                o["max_len"] = max([o["max_len"]] + [w["len"] for w in want])
            for g in gs:
                g.close()
    return out


def branch_tables(k, rng):
    """nodes with 2, 3 and 4 edges on one side, on both sides, an edge below -D, an absent neighbour, a neighbour that is not linear"""
    stem = [rand_seq(rng, k + 8) for _ in range(5)]
    tail = lambda: rand_seq(rng, 12)   # noqa: E731
    seqs = [(stem[0] + b + tail(), 5) for b in "AC"]                               # 2 on the right (or on the left, as the key falls)
    seqs += [(stem[1] + b + tail(), 5) for b in "ACG"]                             # 3
    seqs += [(stem[2] + b + tail(), 5) for b in "ACGT"]                            # 4
    mid = rand_seq(rng, k)
    seqs += [(tail() + a + mid + b + tail(), 5) for a, b in (("A", "C"), ("G", "T"))]   # both sides
    seqs += [(stem[3] + "A" + tail(), 5), (stem[3] + "C" + tail(), 5), (stem[3] + "G" + tail(), 1)]   # the third edge at depth 1 <= -D
    seqs += [(stem[4] + "A" + tail(), 5), (stem[4] + "TA" + tail(), 5), (stem[4] + "TC" + tail(), 5)]  # behind T a node with two edges
    t = make(k, seqs, 1009)
    # an absent neighbour: the first node behind stem[0] + "A" deleted
    key, _ = key_of(t, (stem[0] + "A")[-k:])
    assert t.exist(key) != t.size
    t.deleted[t.exist(key)] = True
    return {"forks": t}


def step_branches(mode):
    out = {}
    o = R.Options()
    for k in ks_of(mode):
        rng = random.Random(200 + k)
        for name, t in branch_tables(k, rng).items():
            slots = [i for i in range(t.size) if t.filled[i]]            # every node, branching or not: the rows are defined for all
            gs = handles(t, mode)
            for cutoff in (100, 3):
                want = [expect_branch_row(t, o, i, side, j, cutoff) for i in slots for side in (0, 1) for j in range(4)]
                got = [g.trace_branches(slots, cutoff) for g in gs]
                compare(got[-1], want, (k, name, cutoff))
                assert len(got) == 1 or same(got[0], got[1]), (k, name, cutoff, "the wide handle differs from the narrow one")
            for g in gs:
                g.close()
            per_side = {}
            for n, i in enumerate(slots):
                for side in (0, 1):
                    rows = want[8 * n + 4 * side:8 * n + 4 * side + 4]
                    per_side.setdefault(sum(1 for w in rows if w["status"] != BELOW), []).append(i)
            both = sum(1 for n in range(len(slots)) if all(sum(1 for w in want[8 * n + 4 * s:8 * n + 4 * s + 4] if w["status"] != BELOW) >= 2 for s in (0, 1)))
            flipped = sum(1 for n, w in enumerate(want) if w["status"] == TRACED and w["direct"] != (1 if (n >> 2) & 1 == 0 else -1))
            kept = sum(1 for n, w in enumerate(want) if w["status"] == TRACED and w["direct"] == (1 if (n >> 2) & 1 == 0 else -1))
            below = 0
            for n, i in enumerate(slots):
                for side in (0, 1):
                    link = t.r_link[i] if side == 0 else t.l_link[i]
                    below += sum(1 for j in range(4) if 0 < R.depth_of(link, j) <= o.D)
            out["k%d_%s" % (k, name)] = {"edges_2": len(per_side.get(2, [])), "edges_3": len(per_side.get(3, [])), "edges_4": len(per_side.get(4, [])),
                                         "both_sides": both, "below": below, "absent": sum(1 for w in want if w["status"] == ABSENT),
                                         "not_linear": sum(1 for w in want if w["status"] == NOT_LINEAR), "flipped": flipped, "kept": kept}
    return out


def step_update(mode):
    """slot 0, slot size - 1 and two slots of one flag byte change on the host; a trace before update() sees the old table, one after
    it the new one"""
    out = {}
    for k in ks_of(mode):
        rng = random.Random(300 + k)
        t = make(k, [(rand_seq(rng, 60 + k + 1), 5) for _ in range(3)], 197)
        assert t.filled[0] and t.filled[t.size - 1]
        reqs = every_request(t)
        slots, directs = [s for s, _ in reqs], [d for _, d in reqs]
        byte = next(b for b in range(1, t.size // 8 - 1) if sum(1 for i in range(8 * b, 8 * b + 8) if t.linear[i]) >= 2)
        x, y = [i for i in range(8 * byte, 8 * byte + 8) if t.linear[i]][:2]
        touched = [0, t.size - 1, x, y]
        before = [expect_walk(t, s, d, 100) for s, d in reqs]
        assert probes_that_wrap(t, before) > 0, (k, "no probe of a walk wraps past the end of the table")
        from dbg_assembly_amd import capi
        for wide in {"narrow": (False,), "wide31": (True,), "above32": (True,)}[mode]:
            t2 = make(k, [], 2)          # a deep copy of t, field by field
            t2.__dict__.update({f: (list(v) if isinstance(v, list) else v) for f, v in t.__dict__.items()})
            host = [np.array(a) for a in arrays_for(t2, wide)]
            with capi.ContigBuilder(k, wide=wide) as g:
                g.set_table(*host)
                host = g._keep          # the arrays the handle reads again: changed in place below
                compare(g.trace(slots, directs, 100), before, (k, "before"))
                # the changes: slot 0 deleted, the last slot's strongest right link one deeper, x deleted, y no longer linear
                t2.deleted[0] = t2.deleted[x] = True
                last = t2.size - 1
                t2.r_link[last] += 1 << ((3 - t2.r_base[last]) * 8)
                t2.linear[y], t2.r_num[y] = False, 2
                new = arrays_for(t2, wide)
                for s in touched:
                    host[0][s] = new[0][s]
                    host[2][s >> 3] = new[2][s >> 3]
                    host[3][s] = new[3][s]
                stale = g.trace(slots, directs, 100)
                compare(stale, before, (k, "changed on the host only"))
                g.update(touched + [x, 0])            # a slot may be listed twice
                after = [expect_walk(t2, s, d, 100) for s, d in reqs]
                compare(g.trace(slots, directs, 100), after, (k, "after update"))
                differ = sum(1 for a, b in zip(before, after) if a != b)
                assert differ > 4, differ
                assert g.simplify_timing()["updated_slots"] == 4
                out["k%d_%s" % (k, "wide" if wide else "narrow")] = {"requests": len(reqs), "differ": differ}
    return out


def step_counts(mode):
    """1, 63, 64, 65 and 257 requests, and the 257 again in batches of 64, at every k of the mode: the same findings at each"""
    outs = [counts_at(k, mode) for k in ks_of(mode)]
    assert all(o == outs[0] for o in outs), outs
    return outs[0]


def counts_at(k, mode):
    rng = random.Random(400 + k)
    t = make(k, [(rand_seq(rng, rng.randrange(1, 12) + k + 1), 5) for _ in range(40)], 1009)
    reqs = every_request(t)
    assert len(reqs) >= 257
    rng.shuffle(reqs)
    want = [expect_walk(t, s, d, 100) for s, d in reqs[:257]]
    out = {}
    gs = handles(t, mode)
    for n in (0, 1, 63, 64, 65, 257):
        for g in gs:
            got = g.trace([s for s, _ in reqs[:n]], [d for _, d in reqs[:n]], 100)
            compare(got, want[:n], (k, n))
            out["n%d" % n] = got[4]["batches"]
    os.environ["DBGK_TEST_HOOKS"] = "simplify_batch=64"
    for g in gs:
        got = g.trace([s for s, _ in reqs[:257]], [d for _, d in reqs[:257]], 100)
        compare(got, want, (k, "batches of 64"))
        out["batched"] = got[4]["batches"]
        got = g.trace_branches([s for s, _ in reqs[:100]], 100)
        compare(got, [expect_branch_row(t, R.Options(), s, side, j, 100) for s, _ in reqs[:100] for side in (0, 1) for j in range(4)], (k, "branches in batches"))
        out["batched_branches"] = got[4]["batches"]
    del os.environ["DBGK_TEST_HOOKS"]
    # the argument checks that need a table: all before device work
    from dbg_assembly_amd import capi
    g = gs[0]
    for bad in (lambda: g.trace([t.size], [1], 100), lambda: g.trace([0], [0], 100), lambda: g.trace([0], [2], 100),
                lambda: g.trace([0], [1], capi.TRACE_MAX_CUTOFF + 1), lambda: g.trace_branches([t.size], 100), lambda: g.update([t.size])):
        try:
            bad()
        except capi.DbgkError as e:
            assert e.status == capi.ERR_ARG, e.status
        else:
            raise AssertionError("a bad argument was accepted")
    with capi.ContigBuilder(k, wide=mode != "narrow") as fresh:
        for call in (lambda: fresh.trace([0], [1], 100), lambda: fresh.trace_branches([0], 100), lambda: fresh.update([0])):
            try:
                call()
            except capi.DbgkError as e:
                assert e.status == capi.ERR_STATE, e.status
            else:
                raise AssertionError("a call before set_table was accepted")
    out["argument_checks"] = 9
    for g in gs:
        g.close()
    return out


if __name__ == "__main__":
    res = {"trace": step_trace, "branches": step_branches, "update": step_update, "counts": step_counts}[sys.argv[1]](sys.argv[2])
    print(json.dumps(res))
