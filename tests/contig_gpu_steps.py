"""GPU steps of tests/test_contig_gpu.py, each run in a child process of its own under a time limit:
    python tests/contig_gpu_steps.py tables | handoff | goldens
Hand-built tables and the golden cases' tables after simplification go through capi.ContigBuilder and are compared with the
restatement's serial read-out: bytes, records, and the number of contigs the host walker read out.  Prints one JSON line of
findings; exits non-zero on a mismatch."""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402

CASES = os.path.join(ROOT, "tests", "golden", "contig_cases")
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
FIELDS = ("anchor", "left_end", "right_end", "left_len", "right_len", "left_depth", "right_depth", "left_mark", "right_mark", "left_repeat",
          "right_repeat", "mid_depth")


def build_table(seqs, k, size):
    """the graph of (sequence, depth) pairs as build_debruijn_graph leaves it (DBGgraph.cpp:76-89, :188-194), nodes inserted in the
    order of their first occurrence; the key-0 node is always there"""
    nodes, order = {0: [0, 0]}, [0]
    mask = (1 << (2 * k)) - 1

    def add(word, base, times):
        sh = (3 - base) * 8
        return word + (min(255, ((word >> sh) & 0xff) + times) - ((word >> sh) & 0xff) << sh)

    for s, times in seqs:
        c = [CODE[x] for x in s]
        kmer = 0
        for p, b in enumerate(c):
            kmer = ((kmer << 2) | b) & mask
            if p < k - 1:
                continue
            left = c[p - k] if p >= k else None
            right = c[p + 1] if p + 1 < len(c) else None
            rc = R.revcomp(kmer, k)
            key, lb, rb = (kmer, left, right) if kmer < rc else (rc, None if right is None else 3 - right, None if left is None else 3 - left)
            if key not in nodes:
                nodes[key] = [0, 0]
                order.append(key)
            if lb is not None:
                nodes[key][0] = add(nodes[key][0], lb, times)
            if rb is not None:
                nodes[key][1] = add(nodes[key][1], rb, times)
    t = R.Table(size, k)
    for key in order:
        t.insert(key, nodes[key][0], nodes[key][1])
    return t


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def check(t, what, want_host=None):
    """t: a table after first_pass (and whatever else changed it) -> summary; asserts the GPU read-out equals the serial one"""
    from dbg_assembly_amd import capi
    want = R.read_out_contigs(t)
    host_nodes = R.order_dependent_nodes(t)
    n_host = sum(1 for c in want if c["anchor"] in host_nodes)
    with capi.ContigBuilder(t.k) as g:
        g.set_table(*t.arrays())
        bases, depths, offsets, rec, summ = g.read_out()
    assert summ["contigs"] == len(want) == len(rec), (what, summ, len(want))
    for i, c in enumerate(want):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        got = {f: int(rec[f][i]) for f in FIELDS}
        assert got == {f: c[f] for f in FIELDS}, (what, i, got, {f: c[f] for f in FIELDS})
        assert bases[lo:hi].tobytes().decode() == c["bases"], (what, i, "bases")
        assert depths[lo:hi].tobytes() == c["depths"], (what, i, "depths")
        assert int(rec["host_walked"][i]) == (1 if c["anchor"] in host_nodes else 0), (what, i, "host_walked")
    assert summ["host_contigs"] == n_host and summ["kernel_contigs"] == len(want) - n_host, (what, summ, n_host)
    assert summ["bytes"] == sum(len(c["bases"]) for c in want)
    if want_host is not None:
        assert (n_host > 0) == want_host, (what, n_host)
    return summ


def step_flips(t):
    """for every step between two live linear nodes: does the walk's direction flip (the neighbour's canonical form is the reverse
    complement)"""
    out = []
    for u in range(t.size):
        if not (t.filled[u] and not t.deleted[u] and t.linear[u]):
            continue
        for d in (1, -1):
            key, flipped = R.canonical(t, R.next_kmer(t, t.kmer[u], t.r_base[u] if d == 1 else t.l_base[u], d))
            if t.is_linear(t.exist(key)):
                out.append(flipped)
    return out


def chain_table(rng, lengths, k, size, depth=5, alphabet="ACGT"):
    """one sequence per chain: n linear nodes between two end nodes that have one side only"""
    t = build_table([(rand_seq(rng, n + k + 1, alphabet), depth) for n in lengths], k, size)
    R.first_pass(t, R.Options())
    return t


def step_tables():
    rng = random.Random(7)
    out = {}
    # chain lengths across wave, block and pointer-jumping-round boundaries; directions flip as the sequence has it
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 4097):
        out["chain_%d" % n] = check(chain_table(rng, [n], 21, 3 * n + 101), "chain %d" % n, False)
        assert out["chain_%d" % n]["kernel_contigs"] == 1
    # no flips at all: k-mers of A and C are smaller than their reverse complements, the walk keeps its direction at every step
    t = chain_table(rng, [300], 31, 1009, alphabet="AC")
    flips = step_flips(t)
    assert len(flips) == 2 * 299 and not any(flips)
    out["no_flip"] = check(t, "no flip", False)
    # a flip at every step: k odd, A or C at even positions and G or T at odd ones, so the k-mers are by turns smaller and larger than
    # their reverse complements; 257 nodes cross a block boundary of the port kernels
    k, n = 21, 257
    seq = "".join(rng.choice("AC" if p % 2 == 0 else "GT") for p in range(n + k + 1))
    t = build_table([(seq, 5)], k, 1009)
    R.first_pass(t, R.Options())
    flips = step_flips(t)
    assert sum(t.linear) == n and len(flips) == 2 * (n - 1) and all(flips)
    out["every_flip"] = check(t, "flip at every step", False)
    # k even with a palindromic k-mer (its own reverse complement, the case nk == rc of the canonical pick) as a linear node
    k = 20
    half = rand_seq(rng, k // 2)
    pal = half + "".join("TGCA"["ACGT".index(c)] for c in reversed(half))
    t = build_table([(rand_seq(rng, 70) + pal + rand_seq(rng, 70), 5)], k, 1009)
    R.first_pass(t, R.Options())
    pkey = sum(CODE[c] << (2 * (k - 1 - j)) for j, c in enumerate(pal))
    assert R.revcomp(pkey, k) == pkey and t.linear[t.exist(pkey)]
    out["palindrome"] = check(t, "palindromic k-mer", None)
    # many chains: anchors at either end and in the middle
    t = chain_table(rng, [rng.randrange(1, 40) for _ in range(200)], 25, 20011)
    summ = check(t, "200 chains", False)
    want = R.read_out_contigs(t)
    kinds = {(c["left_len"] == 1, c["right_len"] == 1) for c in want if c["left_len"] + c["right_len"] > 4}
    assert {(True, False), (False, True), (False, False)} <= kinds, kinds
    out["many"] = summ
    # both ends absent: the end nodes deleted; a deleted neighbour in the middle of a chain cuts it in two
    t = chain_table(rng, [50, 80], 27, 1013)
    for i in range(t.size):
        if t.filled[i] and not t.linear[i] and t.kmer[i]:
            t.deleted[i] = True
    mid = [i for i in range(t.size) if t.linear[i]][40]
    t.deleted[mid] = True
    out["absent"] = check(t, "absent ends", False)
    assert all(c["left_end"] == t.size and c["right_end"] == t.size for c in R.read_out_contigs(t))
    # a repeat: branch ends, Unique and Repeat
    g = rand_seq(rng, 900)
    rep = rand_seq(rng, 60)
    t = build_table([(g[:300] + rep + g[300:600] + rep + g[600:], 6)], 31, 4099)
    R.first_pass(t, R.Options())
    out["repeat"] = check(t, "repeat", False)
    reps = {(c["left_repeat"], c["right_repeat"]) for c in R.read_out_contigs(t)}
    assert any(1 in r for r in reps) and any(2 in r for r in reps), reps
    # depth bytes 10 and 62; an average depth that truncates to 10
    t = build_table([(rand_seq(rng, 120), 10), (rand_seq(rng, 120), 62)], 31, 1021)
    R.first_pass(t, R.Options())
    out["depths"] = check(t, "depths 10 and 62", False)
    assert {c["mid_depth"] for c in R.read_out_contigs(t)} == {9, 61}
    s = rand_seq(rng, 100)
    t = build_table([(s, 10), (s[:60], 1)], 31, 1021)          # depths 10 and 11: the average lies between
    R.first_pass(t, R.Options())
    out["avg_10"] = check(t, "average truncates to 10", False)
    assert [int(c["avg"]) for c in R.read_out_contigs(t)] == [10]
    # no linear node
    t = build_table([(rand_seq(rng, 200), 1)], 31, 1021)       # every link at or below -D
    R.first_pass(t, R.Options())
    out["empty"] = check(t, "no linear node", False)
    assert out["empty"]["contigs"] == 0 and out["empty"]["bytes"] == 0 and out["empty"]["linear_nodes"] == 0
    # 1000 chains of one node
    out["singles"] = check(chain_table(rng, [1] * 1000, 23, 8009), "1000 single nodes", False)
    assert out["singles"]["kernel_contigs"] == 1000
    # a table so full that probe sequences wrap past its last slot
    t = chain_table(rng, [150, 150, 150], 29, 521)
    assert t.filled[t.size - 1] and t.filled[0]
    out["wrap"] = check(t, "probe wrap", False)
    return out


def step_handoff():
    rng = random.Random(11)
    out = {}
    k = 21
    # a cycle of linear nodes
    s = rand_seq(rng, 300)
    t = build_table([(s + s[:k], 5)], k, 1009)
    R.first_pass(t, R.Options())
    out["cycle"] = check(t, "cycle", True)
    # a node whose right neighbour is its own reverse complement (k odd): u + b with u[1:] + b == rc(u)
    half = rand_seq(rng, (k - 1) // 2)
    u = "A" + half + "".join("TGCA"["ACGT".index(c)] for c in reversed(half))
    s = rand_seq(rng, 80) + u + "T"
    t = build_table([(s, 5)], k, 1009)
    R.first_pass(t, R.Options())
    out["self_loop"] = check(t, "self loop", True)
    # the key-0 node as a linear node: poly-A alone, its own neighbour on both sides
    t = build_table([("A" * (k + 6), 5), (rand_seq(rng, 90), 5)], k, 1009)
    R.first_pass(t, R.Options())
    slot0 = t.exist(0)
    assert slot0 != t.size and t.linear[slot0]
    out["key0"] = check(t, "key-0 node", True)
    # a step into another chain that the other chain does not answer: u's right link rewritten to lead to v
    a = rand_seq(rng, 120)
    u = a[50:50 + k]
    other = next(b for b in "ACGT" if b != a[50 + k])
    first = next(b for b in "ACGT" if b != u[0])
    t = build_table([(a, 5), (rand_seq(rng, 40) + first + u[1:] + other + rand_seq(rng, 60), 5)], k, 1009)
    R.first_pass(t, R.Options())
    ukey, flipped = R.canonical(t, sum(CODE[c] << (2 * (k - 1 - j)) for j, c in enumerate(u)))
    slot = t.exist(ukey)
    assert t.linear[slot]
    ob = CODE[other]
    if flipped:      # u's right side is the stored node's left side, complemented
        t.l_link[slot], t.l_base[slot] = 5 << ((3 - (3 - ob)) * 8), 3 - ob
    else:
        t.r_link[slot], t.r_base[slot] = 5 << ((3 - ob) * 8), ob
    out["non_mutual"] = check(t, "non-mutual step", True)
    return out


def step_goldens():
    """the golden cases' tables after simplification: the cap on the hand-off"""
    out = {}
    for f in sorted(os.listdir(CASES)):
        c = R.load_case(os.path.join(CASES, f))
        t = R.Table.from_case(c)
        R.run_stage(t, R.Options.from_args(c["args"]))
        out[f[:-4]] = check(t, f, None if f[0] in "gh" else False)
    return out


if __name__ == "__main__":
    res = {"tables": step_tables, "handoff": step_handoff, "goldens": step_goldens}[sys.argv[1]]()
    print(json.dumps(res))
