"""GPU steps of tests/test_wide_contig_gpu.py, each run in a child process of its own under a time limit:
    python tests/wide_contig_gpu_steps.py tables | shapes | handoff | narrow
Hand-built tables of 128-bit keys (tests/wide_contig_restatement.py) go through capi.ContigBuilder(wide=True) and are compared with
the restatement's serial read-out: bytes, records, and the number of contigs the host walker read out.  Parity is unpinned above
k = 32; at k <= 32 every key has a high word of 0.  Prints one JSON line of findings; exits non-zero on a mismatch."""
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

CODE = W.CODE
KS = (31, 32, 33, 48, 63)
FIELDS = ("anchor", "left_end", "right_end", "left_len", "right_len", "left_depth", "right_depth", "left_mark", "right_mark", "left_repeat",
          "right_repeat", "mid_depth")


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def key_of(s):
    return sum(CODE[c] << (2 * (len(s) - 1 - j)) for j, c in enumerate(s))


def revcomp_text(s):
    return "".join("TGCA"["ACGT".index(c)] for c in reversed(s))


def check(t, what, want_host=None):
    """t: a WideTable after first_pass (and whatever else changed it) -> summary and the five outputs; asserts the GPU read-out equals
    the serial one"""
    from dbg_assembly_amd import capi
    want = W.read_out_contigs(t)
    host_nodes = R.order_dependent_nodes(t)
    n_host = sum(1 for c in want if c["anchor"] in host_nodes)
    with capi.ContigBuilder(t.k, wide=True) as g:
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
    return summ, (bases, depths, offsets, rec)


def step_flips(t):
    """for every step between two live linear nodes: does the walk's direction flip"""
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
    t = W.build_table([(rand_seq(rng, n + k + 1, alphabet), depth) for n in lengths], k, size)
    R.first_pass(t, R.Options())
    return t


def high_words(t):
    return sum(1 for i in range(t.size) if t.filled[i] and t.kmer[i] >> 64)


def step_tables():
    """chain lengths across wave, block and pointer-jumping-round boundaries at every k: below, at and above the word boundary"""
    rng = random.Random(17)
    out = {}
    for k in KS:
        for n in (1, 63, 64, 65, 255, 256, 257, 4097):
            t = chain_table(rng, [n], k, 3 * n + 101)
            assert (high_words(t) > 0) == (k > 32)
            out["k%d_chain_%d" % (k, n)] = check(t, "k %d chain %d" % (k, n), False)[0]
            assert out["k%d_chain_%d" % (k, n)]["kernel_contigs"] == 1
    return out


def step_shapes():
    rng = random.Random(19)
    out = {}
    for k in KS:
        # no flips at all: k-mers of A and C are smaller than their reverse complements
        t = chain_table(rng, [300], k, 1009, alphabet="AC")
        flips = step_flips(t)
        assert len(flips) == 2 * 299 and not any(flips)
        out["k%d_no_flip" % k] = check(t, "k %d no flip" % k, False)[0]
        if k % 2:
            # a flip at every step: k odd, A or C at even positions and G or T at odd ones; 257 nodes cross a block boundary
            n = 257
            seq = "".join(rng.choice("AC" if p % 2 == 0 else "GT") for p in range(n + k + 1))
            t = W.build_table([(seq, 5)], k, 1009)
            R.first_pass(t, R.Options())
            flips = step_flips(t)
            assert sum(t.linear) == n and len(flips) == 2 * (n - 1) and all(flips)
            out["k%d_every_flip" % k] = check(t, "k %d flip at every step" % k, False)[0]
    # k even with a palindromic k-mer (its own reverse complement) as a linear node; odd k has none
    k = 48
    half = rand_seq(rng, k // 2)
    pal = half + revcomp_text(half)
    t = W.build_table([(rand_seq(rng, 70) + pal + rand_seq(rng, 70), 5)], k, 1009)
    R.first_pass(t, R.Options())
    pkey = key_of(pal)
    assert R.revcomp(pkey, k) == pkey and pkey >> 64 and t.linear[t.exist(pkey)]
    out["palindrome"] = check(t, "palindromic k-mer", None)[0]
    # many chains at k = 33 and 63: the anchor's k bytes start at every offset mod 8 of the 8-byte words the emit kernel writes,
    # both counted inside the contig (left_len) and in the output buffer (the contig's first byte + left_len)
    for k in (33, 63):
        t = chain_table(rng, [rng.randrange(1, 40) for _ in range(200)], k, 20011)
        summ, (bases, depths, offsets, rec) = check(t, "k %d, 200 chains" % k, False)
        assert {int(x) % 8 for x in rec["left_len"]} == set(range(8))
        assert {(int(offsets[i]) + int(rec["left_len"][i])) % 8 for i in range(len(rec))} == set(range(8))
        out["k%d_many" % k] = summ
    # a table so full that probe sequences wrap past its last slot, keys with a high word among them
    for k in (33, 63):
        t = chain_table(rng, [150, 150, 150], k, 521)
        assert t.filled[t.size - 1] and t.filled[0] and high_words(t) > 100
        home = [W.hash128(t.kmer[i]) % t.size for i in range(t.size)]
        assert any(t.filled[i] and home[i] > i for i in range(t.size))   # a key whose probe wrapped past the last slot
        out["k%d_wrap" % k] = check(t, "k %d probe wrap" % k, False)[0]
    # a repeat: branch ends, Unique and Repeat, at k = 63
    g = rand_seq(rng, 900)
    rep = rand_seq(rng, 100)
    t = W.build_table([(g[:300] + rep + g[300:600] + rep + g[600:], 6)], 63, 4099)
    R.first_pass(t, R.Options())
    out["k63_repeat"] = check(t, "repeat", False)[0]
    reps = {(c["left_repeat"], c["right_repeat"]) for c in W.read_out_contigs(t)}
    assert any(1 in r for r in reps) and any(2 in r for r in reps), reps
    return out


def step_handoff():
    rng = random.Random(23)
    out = {}
    k = 63
    # a cycle of linear nodes
    s = rand_seq(rng, 300)
    t = W.build_table([(s + s[:k], 5)], k, 1009)
    R.first_pass(t, R.Options())
    out["cycle"] = check(t, "cycle", True)[0]
    # a node whose right neighbour is its own reverse complement (k odd): u + b with u[1:] + b == rc(u)
    half = rand_seq(rng, (k - 1) // 2)
    u = "A" + half + revcomp_text(half)
    t = W.build_table([(rand_seq(rng, 80) + u + "T", 5)], k, 1009)
    R.first_pass(t, R.Options())
    out["self_loop"] = check(t, "self loop", True)[0]
    # the key-0 node as a linear node: poly-A alone, its own neighbour on both sides
    t = W.build_table([("A" * (k + 6), 5), (rand_seq(rng, 130), 5)], k, 1009)
    R.first_pass(t, R.Options())
    slot0 = t.exist(0)
    assert slot0 != t.size and t.linear[slot0]
    out["key0"] = check(t, "key-0 node", True)[0]
    # a step into another chain that the other chain does not answer: u's right link rewritten to lead to v
    a = rand_seq(rng, 200)
    u = a[70:70 + k]
    other = next(b for b in "ACGT" if b != a[70 + k])
    first = next(b for b in "ACGT" if b != u[0])
    t = W.build_table([(a, 5), (rand_seq(rng, 40) + first + u[1:] + other + rand_seq(rng, 80), 5)], k, 1009)
    R.first_pass(t, R.Options())
    ukey, flipped = R.canonical(t, key_of(u))
    slot = t.exist(ukey)
    assert t.linear[slot]
    ob = CODE[other]
    if flipped:      # u's right side is the stored node's left side, complemented
        t.l_link[slot], t.l_base[slot] = 5 << ((3 - (3 - ob)) * 8), 3 - ob
    else:
        t.r_link[slot], t.r_base[slot] = 5 << ((3 - ob) * 8), ob
    out["non_mutual"] = check(t, "non-mutual step", True)[0]
    return out


def step_narrow():
    """k = 31: the wide builder's five outputs on a table of {0, kmer} nodes equal the narrow builder's on the 16-byte table;
    and each kind of handle refuses the other kind's table"""
    from dbg_assembly_amd import capi
    rng = random.Random(29)
    k = 31
    g = rand_seq(rng, 900)
    rep = rand_seq(rng, 60)
    seqs = [(g[:300] + rep + g[300:600] + rep + g[600:], 6)] + [(rand_seq(rng, n + k + 1), 5) for n in (1, 7, 64, 300)]
    s = rand_seq(rng, 200)
    seqs.append((s + s[:k], 5))   # a cycle: the host walker of either handle
    t = W.build_table(seqs, k, 4099)
    R.first_pass(t, R.Options())
    summ, wide = check(t, "k 31", True)
    narrow_t = R.Table(t.size, k)
    narrow_t.__dict__.update(t.__dict__)
    wide_arrays, narrow_arrays = t.arrays(), R.Table.arrays(narrow_t)
    with capi.ContigBuilder(k) as gn:
        gn.set_table(*narrow_arrays)
        narrow = gn.read_out()
        rc = capi.lib().dbgk_wide_contig_set_table(gn._h, t.size, *[x.ctypes.data for x in wide_arrays])
        assert rc == capi.ERR_STATE, rc   # a narrow handle does not take a table of 32-byte nodes
    with capi.ContigBuilder(k, wide=True) as gw:
        rc = capi.lib().dbgk_contig_set_table(gw._h, t.size, *[x.ctypes.data for x in narrow_arrays])
        assert rc == capi.ERR_STATE, rc   # nor a wide handle one of 16-byte nodes
    for a, b in zip(wide[:3], narrow[:3]):
        assert np.array_equal(a, b)
    assert wide[3].tobytes() == narrow[3].tobytes() and summ == narrow[4]
    return {"k31": summ}


if __name__ == "__main__":
    res = {"tables": step_tables, "shapes": step_shapes, "handoff": step_handoff, "narrow": step_narrow}[sys.argv[1]]()
    print(json.dumps(res))
