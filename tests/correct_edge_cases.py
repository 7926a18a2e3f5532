"""Crafted cases for the read corrector (csrc/dbgk_correct.h): reads and tables that sit on the boundaries its own structure
creates -- the 64-bit ballot words of the high/low mask, the 128-window stride of the classify kernel, the 64-candidate chunks of
the one-base fix, the LDS limits on read length (1024) and frontier size (256), the node limit, the trim rule, the smallest and
largest k, and bytes outside ACGTN.  Pure Python, fixed seeds, no GPU and no library load.

scenarios() returns Scenario tuples (name, cat, k, opts, table, table_name, reads, expect, pinned, genome).  `opts` are the
options -m -c -x -n -r; `table` is a SparseTable; `expect` holds one dict per read with the category and the properties the read
was BUILT to have (tests/test_correct_edges_cpu.py checks that the restatement finds exactly those):

    runs          the low runs of the first mask, as (first, last) 0-based k-mer indices
    one_base, tree, deleted, lt, rt, hits    the fields of the result;  lt_gt0 / rt_gt0: the trim is positive
    out           the corrected full-length read
    path          0 classify, 1 the LDS kernel, 2 the overflow kernel (where the construction fixes it)
    max_frontier  the largest frontier any tree of the read accepted;  depth0: frontiers the first tree accepted
    zero_word / full_word    the mask word that is all low / exactly all high;  low_at: a window that must count as low
    both_ext      both extension trees corrected

A scenario whose name ends in _unpinned is never sent to the real reference (k = 1 has no table file, k = 19 needs a 32 GiB
table, and the reference indexes out of bounds on a window that starts with a byte outside ACGTN); every other one is pinned
by tests/golden/correct_edges, which tests/golden/make_correct_edges_golden.py writes."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_restatement as CR  # noqa: E402

Scenario = namedtuple("Scenario", "name cat k opts table table_name reads expect pinned genome")

N_DEFAULT = 5000000
LDS_NODES, LDS_READ_LEN = 256, 1024            # kLdsNodes, kLdsReadLen
BLOCK = 4096                                   # bytes of raw table per sparse upload
CATEGORIES = ["mask_words", "runs", "classify", "one_base_chunks", "lds_length", "frontier_cap", "node_limit", "trim_x",
              "small_k", "large_k", "odd_bytes"]   # batch_shape reuses the mask_words scenario (tests/correct_gpu_steps.py)
MASK_NKS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)
MASK_EDGES = (62, 63, 64, 65, 126, 127, 128, 129)
CLASSIFY_NKS = (128, 129, 130, 256, 257)
CAP_MS = (252, 255, 258)
NODE_LIMIT_DEPTH = 40


def rcv(v, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (v & 3))
        v >>= 2
    return r


def kmer_values(seq, k):
    """seq2bit of every window of seq (ACGT only)"""
    out, v, full = [], 0, (1 << (2 * k)) - 1
    for i, b in enumerate(seq):
        v = ((v << 2) | CR.ALPHA[b]) & full
        if i >= k - 1:
            out.append(v)
    return out


class SparseTable(CR.Table):
    """the LOADED table (after the loader's mirror) as a set of values, usable at any k without 4^k bits: `both` holds the listed
    canonical values and their reverse complements; they are the high ones, or with inverted=True ("all ones except ...") the only
    low ones.  The raw file holds the canonical values only (inverted: every bit but the listed pairs); the mirror restores the rest."""

    def __init__(self, k, values, inverted=False):
        self.k, self.total, self.bits, self.inverted = k, 4 ** k, b"", inverted
        self.canon = {min(v, rcv(v, k)) for v in values}
        self.both = self.canon | {rcv(v, k) for v in self.canon}

    def hi(self, v):
        return v < self.total and ((v in self.both) != self.inverted)

    def table_bytes(self):
        return max(self.total // 8, 1)

    def n_canonical(self):
        """set values v with v <= rc(v): what the loader and seal() count (Kmer_hifreq_num)"""
        if not self.inverted:
            return len(self.canon)
        palindromes = 4 ** (self.k // 2) if self.k % 2 == 0 else 0
        return (self.total + palindromes) // 2 - len(self.canon)

    def raw_block(self, first_byte, n_bytes, loaded=False):
        """raw file bytes [first_byte, first_byte + n_bytes): bit v is bit 7 - v % 8 of byte v / 8; loaded: after the mirror"""
        blk = np.full(n_bytes, 0xFF if self.inverted else 0, dtype=np.uint8)
        lo, hi = first_byte * 8, (first_byte + n_bytes) * 8
        for v in (self.both if self.inverted or loaded else self.canon):
            if lo <= v < hi:
                if self.inverted:
                    blk[(v >> 3) - first_byte] &= ~(0x80 >> (v & 7)) & 0xFF
                else:
                    blk[(v >> 3) - first_byte] |= 0x80 >> (v & 7)
        return blk

    def raw_blocks(self):
        """(first_byte, bytes) of every 4 KiB block of the raw file that holds a set bit"""
        nb = self.table_bytes()
        if self.inverted:
            for at in range(0, nb, BLOCK):
                yield at, self.raw_block(at, min(BLOCK, nb - at))
            return
        by_block = {}
        for v in self.canon:
            by_block.setdefault(v >> 15, []).append(v)
        for b in sorted(by_block):
            at = b * BLOCK
            blk = np.zeros(min(BLOCK, nb - at), dtype=np.uint8)
            for v in by_block[b]:
                blk[(v >> 3) - at] |= 0x80 >> (v & 7)
            yield at, blk

    def raw_bytes(self):
        """the whole raw file (k <= 17)"""
        raw = np.full(self.table_bytes(), 0xFF if self.inverted else 0, dtype=np.uint8)
        for at, blk in self.raw_blocks():
            raw[at:at + blk.size] = blk
        return raw


def params_of(scn):
    return CR.Params(k=scn.k, **scn.opts)


def opts(m=17, c=2, x=17, n=N_DEFAULT, r=75):
    return dict(m=m, c=c, x=x, n=n, r=r)


K13 = dict(m=13, c=2, x=5, r=30)


def other(b, rng):
    """a base whose code differs from byte b's"""
    return b"ACGT"[(CR.ALPHA[b] % 4 + 1 + int(rng.integers(3))) % 4]


def rand_seq(rng, n):
    return bytes(b"ACGT"[v] for v in rng.integers(0, 4, n))


class Build:
    """a scenario on a random genome: every read is cut from a locus of its own; the table is the genome's k-mers, minus
    `removed`, plus `added` (byte strings of k bases)"""

    def __init__(self, name, cat, k, o, seed, room=70000, pinned=True, table_name=None):
        self.name, self.cat, self.k, self.o, self.pinned, self.table_name = name, cat, k, o, pinned, table_name or name
        self.rng = np.random.default_rng(seed)
        self.g = bytearray(rand_seq(self.rng, room))
        self.cursor, self.reads, self.expect, self.removed, self.added = 0, [], [], [], []

    def locus(self, n):
        a = self.cursor
        self.cursor += n + 1
        assert self.cursor + self.k < len(self.g)
        return a

    def cut(self, n):
        a = self.locus(n)
        return a, bytearray(self.g[a:a + n])

    def sub(self, read, *positions):
        for p in positions:
            read[p] = other(read[p], self.rng)
        return read

    def junk(self, n, at=None):
        """n random bases; with `at`, in place of genome[at:at + n] and unlike it in the first and the last base"""
        j = bytearray(rand_seq(self.rng, n))
        if at is not None:
            for i in (0, n - 1):
                if j[i] == self.g[at + i]:
                    j[i] = other(j[i], self.rng)
        return bytes(j)

    def add(self, read, **expect):
        self.reads.append(bytes(read))
        self.expect.append(dict(cat=self.cat, **expect))

    def finish(self):
        genome = bytes(self.g[:self.cursor + self.k])
        vals = set(kmer_values(genome, self.k))
        vals -= {CR.seq2bit(w) for w in self.removed} | {rcv(CR.seq2bit(w), self.k) for w in self.removed}
        vals |= {CR.seq2bit(w) for w in self.added}
        return Scenario(self.name, self.cat, self.k, opts(**self.o), SparseTable(self.k, vals), self.table_name, self.reads,
                        self.expect, self.pinned, genome)


def clean(g):
    return dict(one_base=0, tree=0, lt=0, rt=0, out=bytes(g))


def _mask_words():
    k = 13
    B = Build("mask_words", "mask_words", k, K13, 101)
    for nk in MASK_NKS:                     # all high
        a, r = B.cut(nk + k - 1)
        B.add(r, nk=nk, runs=[], path=0, deleted=int(nk < 13 or len(r) < 30), **clean(r))
    for nk in MASK_NKS:                     # one interior substitution: a low run of exactly k, one end of it on a word edge
        for t in MASK_EDGES:
            for which in ("first", "last"):
                p = t + k - 1 if which == "first" else t
                if not k <= p <= nk - 2:
                    continue
                a, r = B.cut(nk + k - 1)
                g = bytes(r)
                B.add(B.sub(r, p), nk=nk, edge=(which, t), runs=[(p - k + 1, p)], path=1, deleted=0, **dict(clean(g), one_base=1))
    a, r = B.cut(129 + k - 1)               # a run wholly inside word 0
    g = bytes(r)
    B.add(B.sub(r, 22), nk=129, inside_word=0, runs=[(10, 22)], path=1, deleted=0, **dict(clean(g), one_base=1))
    a = B.locus(250)                        # a whole word of zeros between two regions
    B.add(B.g[a:a + 60] + B.junk(90, a + 60) + B.g[a + 150:a + 250], zero_word=1, runs=[(48, 149)], one_base=0, path=1)
    a = B.locus(64 + 76 + 20)               # the high k-mers fill word 1 exactly
    B.add(B.junk(64, a) + B.g[a + 64:a + 140] + B.junk(20, a + 140), full_word=1, runs=[(0, 63), (128, 147)], one_base=0, path=1)
    return B.finish()


def _runs(c):
    k, m, L = 13, 13, 150
    B = Build("runs_c%d" % c, "runs", k, dict(K13, c=c), 202, table_name="runs")

    def add(r, g, **e2):
        """e2: what holds at -c 2; at -c 0 nothing is touched"""
        if c == 0:
            e2 = dict(e2, one_base=0, tree=0, out=bytes(r))
            for key in ("both_ext", "lt", "rt", "rt_gt0", "lt_gt0", "deleted"):
                e2.pop(key, None)
        B.add(r, **e2)

    for d in (1, k - 1, k, k + 1):          # two substitutions d apart
        a, r = B.cut(L)
        g = bytes(r)
        B.sub(r, 60, 60 + d)
        if d <= k:
            add(r, g, two_subs=d, runs=[(48, 60 + d)], deleted=0, **dict(clean(g), tree=2))
        else:
            add(r, g, two_subs=d, runs=[(48, 60), (62, 74)], deleted=0, **dict(clean(g), one_base=2))
    for p, touches in ((k - 1, True), (k, False), (L - k, True), (L - k - 1, False)):   # k - 1 and k bases from a read end
        a, r = B.cut(L)
        g = bytes(r)
        B.sub(r, p)
        lo, hi = max(p - k + 1, 0), min(p, L - k)
        add(r, g, end_distance=(p, touches), runs=[(lo, hi)], deleted=0, **dict(clean(g), **({"tree": 1} if touches else {"one_base": 1})))
    a, r = B.cut(L)                         # a run of k - 1: the first window over the error is in the table, so no one-base fix
    g = bytes(r)
    B.sub(r, 60)
    B.added.append(bytes(r[48:61]))
    add(r, g, short_run=k - 1, runs=[(49, 60)], deleted=0, **dict(clean(g), tree=1))
    a, r = B.cut(L)                         # both extension trees correct
    g = bytes(r)
    add(B.sub(r, k - 1, L - k), g, both_ext=1, runs=[(0, k - 1), (L - 2 * k + 1, L - k)], deleted=0, **dict(clean(g), tree=2))
    a, r = B.cut(L)                         # three separated errors: the third one needs -c 3
    g = bytes(r)
    B.sub(r, 30, 70, 110)
    if c >= 3:
        add(r, g, three=1, runs=[(18, 30), (58, 70), (98, 110)], deleted=0, **dict(clean(g), one_base=3))
    else:
        add(r, g, three=1, runs=[(18, 30), (58, 70), (98, 110)], deleted=0, one_base=2, tree=0, lt=0, rt_gt0=True,
            out=g[:110] + bytes(r[110:111]) + g[111:])
    a, r = B.cut(L)                         # a two-edit tree, then an error at the read end that has one change left at -c 3
    g = bytes(r)
    B.sub(r, 60, 61, L - k)
    if c >= 3:
        add(r, g, two_then_one=1, runs=[(48, 61), (L - 2 * k + 1, L - k)], deleted=0, **dict(clean(g), tree=3))
    else:
        add(r, g, two_then_one=1, runs=[(48, 61), (L - 2 * k + 1, L - k)], deleted=0, one_base=0, tree=2, lt=0, rt_gt0=True,
            out=g[:L - k] + bytes(r[L - k:L - k + 1]) + g[L - k + 1:])
    return B.finish()


def _runs_m():
    """high regions of m - 1, m and m + 1 k-mers between two two-base errors, at -c 4: the region counts from m on"""
    k, m, L = 13, 13, 150
    B = Build("runs_c4_m", "runs", k, dict(K13, c=4), 203)
    for h in (m - 1, m, m + 1):
        a, r = B.cut(L)
        g = bytes(r)
        p2 = 41 + k + h
        B.sub(r, 40, 41, p2, p2 + 1)
        e = dict(between=h, runs=[(28, 41), (p2 - k + 1, p2 + 1)], deleted=0, one_base=0, rt=0)
        if h < m:
            B.add(r, tree=2, lt_gt0=True, out=bytes(r[:p2]) + g[p2:], **e)
        else:
            B.add(r, tree=4, lt=0, out=g, **e)
    return B.finish()


def _classify():
    k, m = 13, 13
    B = Build("classify", "classify", k, dict(K13, r=20), 303)
    for nk in CLASSIFY_NKS:
        a, r = B.cut(nk + k - 1)
        B.add(r, nk=nk, runs=[], path=0, deleted=0, **clean(r))
        for idx in sorted({0, 63, 64, 127, 128, nk - 1}):   # one k-mer taken out of the table
            if idx < nk:
                a, r = B.cut(nk + k - 1)
                B.removed.append(bytes(r[idx:idx + k]))
                B.add(r, nk=nk, low_index=idx, runs=[(idx, idx)], path=1, one_base=0)
    for p, idx in ((0, 0), (129 + k - 2, 128)):          # a substitution in the first / last base
        a, r = B.cut(129 + k - 1)
        B.add(B.sub(r, p), nk=129, low_index=idx, runs=[(idx, idx)], path=1, one_base=0)
    for nk, deleted in ((m - 1, 1), (m, 0)):
        a, r = B.cut(nk + k - 1)
        B.add(r, nk=nk, runs=[], path=0, deleted=deleted, **clean(r))
    for L in (0, k - 1, k):
        a, r = B.cut(L)
        B.add(r, length=L, runs=[], path=0, deleted=1, **clean(r))
    B.add(B.junk(k), length=k, runs=[(0, 0)], path=1, deleted=1, one_base=0, tree=0)
    return B.finish()


def _one_base_chunks(k):
    L, p = 100, 50
    B = Build("one_base_chunks_k%d" % k, "one_base_chunks", k, {}, 400 + k)

    def place(true, err, passing):
        """a read with byte err at p where the genome has `true`; the table loses true's k windows and gains, per (base, j)
        of `passing`, the base's windows except window j (j None: all of them)"""
        a = B.locus(L)
        B.g[a + p] = true
        r = bytearray(B.g[a:a + L])
        s = p - k + 1
        B.removed.extend(bytes(r[s + j:s + j + k]) for j in range(k))
        for b, skip in passing:
            w = bytearray(r)
            w[p] = b
            B.added.extend(bytes(w[s + j:s + j + k]) for j in range(k) if j != skip)
        g = bytes(r)
        r[p] = err
        return r, g

    for bi, b in enumerate(b"ACGT"):        # candidate b has every window but j
        for j in range(k):
            err = b"ACGT"[(bi + 1 + j % 3) % 4]
            true = b if j % 2 == 0 else next(c for c in b"ACGT" if c != b and c != err)
            r, g = place(true, err, [(b, j)])
            B.add(r, lacks=(chr(b), j), runs=[(p - k + 1, p)], one_base=0, path=1)
    trios = ((b"T", b"C", b"A"), (b"G", b"A", b"T"), (b"C", b"A", b"G"), (b"T", b"G", b"C"))
    for j in range(k):                      # an earlier decoy lacks window j only; the true base passes
        true, decoy, err = (t[0] for t in trios[j % 4])
        r, g = place(true, err, [(decoy, j), (true, None)])
        B.add(r, decoy=(chr(decoy), j), runs=[(p - k + 1, p)], path=1, deleted=0, **dict(clean(g), one_base=1))
    r, g = place(ord("T"), ord("A"), [(ord("C"), None), (ord("T"), None)])   # two bases pass: the earlier one, C, is taken
    B.add(r, two_pass=1, runs=[(p - k + 1, p)], one_base=1, tree=0, lt=0, rt=0, deleted=0, path=1, out=g[:p] + b"C" + g[p + 1:])
    r, g = place(ord("C"), ord("g"), [(ord("C"), None)])
    B.add(r, err_byte="g", runs=[(p - k + 1, p)], path=1, deleted=0, **dict(clean(g), one_base=1))
    r, g = place(ord("G"), ord("N"), [(ord("G"), None)])
    B.add(r, err_byte="N", runs=[(p - k + 1, p)], path=1, deleted=0, **dict(clean(g), one_base=1))
    return B.finish()


def _lds_length():
    k = 13
    B = Build("lds_length", "lds_length", k, K13, 505)
    for L in (LDS_READ_LEN - 1, LDS_READ_LEN, LDS_READ_LEN + 1):
        path = 1 if L <= LDS_READ_LEN else 2
        a, r = B.cut(L)
        g = bytes(r)
        B.add(B.sub(r, 1005), length=L, runs=[(993, 1005)], path=path, deleted=0, **dict(clean(g), one_base=1))
        a, r = B.cut(L)
        g = bytes(r)
        B.add(B.sub(r, 1003, 1004), length=L, runs=[(991, 1004)], path=path, deleted=0, **dict(clean(g), tree=2))
    return B.finish()


def _cap_read(k, M):
    """all ones except one k-mer of the read's middle: at -c 1 the gap tree's frontier grows by 3 a cycle for M / 3 cycles"""
    rng = np.random.default_rng(600 + k)
    read = rand_seq(rng, 2 * CAP_MS[-1] + k + 40)[:2 * M + k + 40]
    mid = M + 20
    return read, mid, SparseTable(k, [CR.seq2bit(read[mid:mid + k])], inverted=True)


def _frontier_cap(k, M):
    read, mid, T = _cap_read(k, M)
    top = 1 + 3 * (M // 3)
    e = dict(cat="frontier_cap", runs=[(mid, mid)], max_frontier=top, path=1 if top <= LDS_NODES else 2, hits=0, one_base=0)
    return Scenario("frontier_cap_k%d_M%d" % (k, M), "frontier_cap", k, opts(m=M, c=1), T, "ones_k%d_M%d" % (k, M), [read], [e], True, read)


@functools.lru_cache(maxsize=None)
def node_limit_count(depth=NODE_LIMIT_DEPTH):
    """the cumulative node count at which the first (gap) tree of the k = 9, M = 255 capacity read would take its frontier of
    `depth`, as the restatement's observer reports it at the default -n"""
    read, mid, T = _cap_read(9, 255)
    trees = []
    CR.correct_one_read(read, T, CR.Params(k=9, **opts(m=255, c=1)), trees)
    assert trees[0]["right"] and not trees[0]["modify"] and len(trees[0]["frontiers"]) > depth
    return trees[0]["cum"][depth - 1]


def _node_limit(extra):
    """the M = 255 read of frontier_cap with -n at the count its gap tree reaches at depth 40 (+ extra).  Three trees run: the
    gap tree rightward from the left region, the gap tree leftward from the right region, and -- both having failed -- the right
    extension tree, which starts where the first one did.  Each grows by about 3 nodes a cycle for M / 3 = 85 cycles, far beyond
    the count, so each of them reaches it: one hit apiece, at depth 40 (+ extra) in the first."""
    k, M = 9, 255
    read, mid, T = _cap_read(k, M)
    n = node_limit_count() + extra
    e = dict(cat="node_limit", runs=[(mid, mid)], hits=3, depth0=NODE_LIMIT_DEPTH - 1 + extra, path=1, one_base=0, tree=0)
    return Scenario("node_limit_plus%d" % extra, "node_limit", k, opts(m=M, c=1, n=n), T, "ones_k9_M255", [read], [e], True, read)


def _trim_x(x):
    k, L = 13, 150
    B = Build("trim_x%d" % x, "trim_x", k, dict(K13, x=x), 700, table_name="trim_x")
    two = x > k - 1    # beyond k - 1 bases from the end a single substitution is a one-base fix: two adjacent ones need the tree
    for q, trims in ((x, True), (x + 1, False)):                  # 1-based position of the edit nearest the left end
        a, r = B.cut(L)
        g = bytes(r)
        B.sub(r, *((q - 1, q) if two else (q - 1,)))
        B.add(r, left_edit=q, deleted=0, **dict(clean(g), tree=2 if two else 1, lt=x if trims else 0))
    for q, trims in ((L - x + 1, True), (L - x, False)):          # ... nearest the right end
        a, r = B.cut(L)
        g = bytes(r)
        B.sub(r, *((q - 2, q - 1) if two else (q - 1,)))
        B.add(r, right_edit=q, deleted=0, **dict(clean(g), tree=2 if two else 1, rt=x if trims else 0))
    return B.finish()


def _trim_clamp():
    """lt + x exceeds L: 20 junk bases, then 25 of the genome (m k-mers); the left tree stops in the junk"""
    B = Build("trim_clamp", "trim_x", 13, dict(K13, x=40), 777)
    a = B.locus(45)
    B.add(B.junk(20, a) + B.g[a + 20:a + 45], clamp=1, runs=[(0, 19)], one_base=0, lt=45, rt=0, deleted=1)
    return B.finish()


def _small_k(k):
    rng = np.random.default_rng(800 + k)
    canon = sorted({min(v, rcv(v, k)) for v in range(4 ** k)})
    picked = [canon[i] for i in rng.permutation(len(canon))[:max(1, round(0.6 * len(canon)))]]
    T = SparseTable(k, picked)
    reads = [rand_seq(rng, (k, k + 1, 30, 64, 65, 100)[i % 6]) for i in range(60)]
    name = "small_k%d" % k + ("_unpinned" if k == 1 else "")
    return Scenario(name, "small_k", k, opts(m=3, x=2, r=5), T, name, reads, [dict(cat="small_k") for _ in reads], k > 1, b"")


def _large_k():
    k, L = 19, 150
    B = Build("k19_parity_unpinned", "large_k", k, {}, 919, pinned=False)
    for i in range(8):
        a, r = B.cut(L)
        B.add(r, runs=[], path=0, deleted=0, **clean(r))
    for i in range(12):
        a, r = B.cut(L)
        g = bytes(r)
        p = 25 + 9 * i
        B.add(B.sub(r, p), runs=[(p - k + 1, p)], path=1, deleted=0, **dict(clean(g), one_base=1))
    for i in range(6):
        a, r = B.cut(L)
        g = bytes(r)
        p = 40 + 11 * i
        B.add(B.sub(r, p, p + 1), runs=[(p - k + 1, p + 1)], path=1, deleted=0, **dict(clean(g), tree=2))
    for p in (k - 1, L - k, 3, L - 2):
        a, r = B.cut(L)
        g = bytes(r)
        B.add(B.sub(r, p), runs=[(max(p - k + 1, 0), min(p, L - k))], path=1, deleted=0, out=g, one_base=0, tree=1)
    for i in range(10):                     # random substitutions, 2 %
        a, r = B.cut(L)
        B.add(B.sub(r, *[int(v) for v in np.flatnonzero(B.rng.random(L) < 0.02)]))
    return B.finish()


ODD = b"X.-R"


def _odd_bytes():
    """one genome, two scenarios: (a) the byte lies within the last k - 1 bases, so it is never the first byte of a window
    (reference-pinned); (b) it starts a window, or is >= 128 (the reference indexes out of bounds: unpinned)"""
    k, L = 13, 150
    nk = L - k + 1
    B = Build("odd_bytes", "odd_bytes", k, K13, 1001)
    tail = []
    for b in ODD:
        for p in (nk, nk + 5, L - 1):
            a, r = B.cut(L)
            r[p] = b
            B.add(r, odd=(chr(b), p))
            tail.append(len(B.reads) - 1)
    for b in ODD:
        for p in (0, 70, nk - 1):           # the window that starts with the byte has a value >= 4^k: low
            a, r = B.cut(L)
            r[p] = b
            B.add(r, odd=(chr(b), p), low_at=p, path=1)
    for b in (128, 200, 255):
        for p in (70, L - 1):
            a, r = B.cut(L)
            r[p] = b
            B.add(r, odd=(b, p), **(dict(low_at=p, path=1) if p < nk else {}))
    s = B.finish()
    rest = [i for i in range(len(s.reads)) if i not in tail]
    return [s._replace(name=name, pinned=pinned, reads=[s.reads[i] for i in idx], expect=[s.expect[i] for i in idx])
            for name, pinned, idx in (("odd_bytes_tail", True, tail), ("odd_bytes_unpinned", False, rest))]


@functools.lru_cache(maxsize=None)
def scenarios():
    out = [_mask_words(), _runs(0), _runs(2), _runs(3), _runs_m(), _classify()]
    out += [_one_base_chunks(k) for k in (15, 16, 17)]
    out.append(_lds_length())
    out += [_frontier_cap(k, M) for k in (9, 13) for M in CAP_MS]
    out += [_node_limit(0), _node_limit(1), _trim_x(5), _trim_x(17), _trim_clamp()]
    out += [_small_k(k) for k in (1, 2, 3, 4)]
    out.append(_large_k())
    out += _odd_bytes()
    assert len({s.name for s in out}) == len(out)
    return out


def scenario(name):
    return next(s for s in scenarios() if s.name == name)


def first_mask(read, T, k):
    return [1 if T.hi(CR.seq2bit(read[i:i + k])) else 0 for i in range(max(len(read) - k + 1, 0))]


def low_runs(mask):
    return [(s - 1, e - 1) for s, e in CR._runs(mask, 0)]


def restate_read(read, T, P, correct_one_read=CR.correct_one_read):
    """the restatement's answer for one read, with what the kernels add to it: the path"""
    trees = []
    out, one, multi, deleted, lt, rt, hits = correct_one_read(read, T, P, trees)
    mask = first_mask(read, T, P.k)
    top = max([f for t in trees for f in t["frontiers"]], default=0)
    path = 0 if 0 not in mask else 2 if len(read) > LDS_READ_LEN or top > LDS_NODES else 1
    return dict(out=out, one_base=one, tree=multi, deleted=deleted, lt=lt, rt=rt, hits=hits, path=path, mask=mask,
                runs=low_runs(mask), max_frontier=top, trees=trees)


@functools.lru_cache(maxsize=None)
def restated(name):
    """restate_read of every read of a scenario (computed once, shared by the tests; treat as read-only)"""
    s = scenario(name)
    P = params_of(s)
    return [restate_read(r, s.table, P) for r in s.reads]


def headers(scn):
    return [b">%s_%d" % (scn.name.encode(), i) for i in range(len(scn.reads))]


def reads_file(scn):
    """the FASTA file of a scenario (pinned ones only hold bytes a text file can carry)"""
    return b"".join(b"%s\n%s\n" % (h, r) for h, r in zip(headers(scn), scn.reads))
