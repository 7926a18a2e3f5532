"""Crafted cases for the map kernel (csrc/dbgk_map.h): reads that sit on the boundaries its own structure creates -- the chunks
of the seed scan, the LDS slice and its dword staging, the 64-wide strides of the two extension loops, the identity table, the
gate of the second alignment, the length tests and the letters outside ACGTacgtNn.  Pure Python, fixed seeds, no GPU and no
library load.  scenarios() returns Scenario tuples (name, k, s, r, identity, second, contigs, reads, expect); `expect` holds one
dict per read with the properties the read was BUILT to have:

    cat        the category the read belongs to (CATEGORIES lists them all)
    skipped    the read is too short to be mapped (L < r or L < k + s): two empty hits
    seed       0-based start of the window that must seed the first alignment (None: nothing seeds)
    direct     "F" / "R";  contig: index of the contig hit (where it matters)
    left/right bases the alignment is extended towards the contig's start / end, in the contig's orientation
    mis        mismatches counted in the two extensions;  accepted: whether the identity test lets the first hit through
    second     "none" (two empty fields), "hit" (found and accepted) or "rejected" (found, contig = -1)
    batch      (only in the scenario of the growing identity table) the batch the read goes in, 0 or 1
    first_window, ext, limit, offset_mod4, partner: what a category is counted by (tests/test_map_edges_cpu.py)

Every read is built from a contig slice: forward position j of the read lies on contig position a + j, positions outside the
contig hold junk.  Windows below the intended seed are destroyed by substitutions k - 1 apart, so the first window that can
seed, both extension lengths and the number of mismatches follow from the construction alone.  tests/test_map_edges_cpu.py
checks that the restatement (tests/map_restatement.py) finds exactly that; tests/map_gpu_steps.py holds the kernel to the
restatement."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import map_restatement as MR  # noqa: E402

Scenario = namedtuple("Scenario", "name k s r identity second contigs reads expect")

PARAMS = [(31, 5), (21, 5), (15, 40), (31, 1), (2, 1)]
GOLDEN_PARAMS = PARAMS[:4]                     # what goes to the real reference (tests/golden/map_edge_cases)
RAMPS = (1, 4, 64)                             # first chunks of the seed scan that the GPU step runs
FIRST_WINDOWS = sorted({c + d for c in RAMPS for d in (-1, 0, 63, 64, 127, 128)})
EXT_LENGTHS = (0, 1, 63, 64, 65, 129)
SLICE = 1024                                   # kMapSlice: the longest read that is mapped out of LDS
STAGED = (1023, 1024, 1025, 1100)
CATEGORIES = ["ramp", "two_seeds", "partner_missing", "partner_dup", "partner_other_contig", "inverted", "staging", "tiny",
              "ext_read_end", "ext_contig_end", "flush", "ext_mismatch_stride2", "ext_mismatch_last", "identity_edge",
              "accept_growth", "second_gate", "second_first_rejected", "second_rejected", "second_off", "length_edge", "below_r",
              "empty", "lower_case", "N", "key0", "other_first", "other_last", "other_ext", "high_bytes", "k2"]

_COMP = bytes(c if c in b"Nn" else b"TGCAN"[MR._CODE[c]] for c in range(256))


def rc(seq):
    return bytes(seq)[::-1].translate(_COMP)


def rand_seq(rng, n):
    return bytes(b"ACGT"[v] for v in rng.integers(0, 4, n))


def other(c):
    """a base that differs from byte c in its code"""
    return b"ACGT"[(MR._CODE[c] + 1) % 4] if MR._CODE[c] < 4 else ord("C")


def base_contigs(k, s):
    """[main, dup1, dup2, joinA, joinB, periodic, polyA]: a long random contig; two that share a 70-base stretch (its k-mers are
    not unique); two that share a stretch of k - s bases (a window of the one and its partner window of the other fit in one
    read); a stretch of period 2s (an inverted seed); a single all-A window (key 0).  The bases beside a
    shared stretch differ between its two contigs, so that no window over its edge is shared by chance"""
    rng = np.random.default_rng(1000 * k + s)
    dup = rand_seq(rng, 70)
    join = rand_seq(rng, max(k - s, 0))
    unit = rand_seq(rng, 2 * s)
    while unit[:s] == unit[s:] or rc(unit) == unit:
        unit = rand_seq(rng, 2 * s)
    period = (unit * (k + s))[:k + s] if k >= 2 * s else b""
    return [rand_seq(rng, 1500), rand_seq(rng, 199) + b"A" + dup + b"C" + rand_seq(rng, 299), rand_seq(rng, 149) + b"G" + dup + b"T" + rand_seq(rng, 99),
            rand_seq(rng, 199) + b"A" + join + b"C" + rand_seq(rng, 199), rand_seq(rng, 199) + b"G" + join + b"T" + rand_seq(rng, 399),
            rand_seq(rng, 100) + b"C" + period + b"G" + rand_seq(rng, 100), rand_seq(rng, 150) + b"C" + b"A" * k + b"G" + rand_seq(rng, 250)]


MAIN, DUP1, DUP2, JOIN_A, JOIN_B, PERIODIC, POLYA = range(7)


class Builder:
    def __init__(self, name, k, s, r=0, identity=0.9, second=False, contigs=None):
        self.name, self.k, self.s, self.r, self.identity, self.second = name, k, s, r, identity, second
        self.contigs = contigs if contigs is not None else base_contigs(k, s)
        self.rng = np.random.default_rng(7 + sum(name.encode()))
        self.reads, self.expect = [], []

    def add(self, read, cat, **intent):
        self.reads.append(bytes(read))
        self.expect.append(dict(intent, cat=cat))

    def skip(self, read, cat, **more):
        self.add(read, cat, skipped=True, seed=None, second="none", **more)

    def intent(self, read, cid, a, direct, seed, mis=None, **more):
        """what a read aligned at offset a of contig cid and seeded at window `seed` must give; `mis` (the number of bytes the
        construction changed inside the extensions) is asserted against a byte-for-byte comparison"""
        k, s, L, C = self.k, self.s, len(read), self.contigs[cid]
        fwd = bytes(read) if direct == "F" else rc(read)
        lo, hi = max(0, -a), min(L, len(C) - a)
        f = seed if direct == "F" else L - seed - s - k
        assert lo <= f and f + s + k <= hi, (self.name, "the seed lies outside the contig")
        diff = sum(fwd[j] != C[a + j] for j in list(range(lo, f)) + list(range(f + s + k, hi)))
        assert mis is None or mis == diff, (self.name, mis, diff)
        left, right = f - lo, hi - f - s - k
        return dict(dict(seed=seed, direct=direct, contig=cid, left=left, right=right, mis=diff, second="none",
                         accepted=MR.accepted(diff, k + s + left + right, self.identity)), **more)

    def aligned(self, cid, a, L, direct, seed=0, extra=(), junk=None):
        """-> (read, number of changed bytes on the contig): forward position j lies on contig position a + j; read windows
        below `seed` are destroyed by substitutions k - 1 apart, `extra` are further substitutions (positions of the read)"""
        C = self.contigs[cid]
        fwd = bytearray(C[a + j] if 0 <= a + j < len(C) else (junk if junk is not None else b"ACGT"[int(self.rng.integers(0, 4))])
                        for j in range(L))
        read = bytearray(fwd if direct == "F" else rc(fwd))
        subs = sorted(set(range(seed - 1, -1, -max(self.k - 1, 1))) | set(extra))
        for p in subs:
            read[p] = other(read[p])
        on_contig = sum(0 <= a + (p if direct == "F" else L - 1 - p) < len(C) for p in subs)
        return read, on_contig

    def put(self, cat, cid, a, L, direct, seed=0, extra=(), junk=None, **more):
        read, n = self.aligned(cid, a, L, direct, seed, extra, junk)
        self.add(read, cat, **self.intent(read, cid, a, direct, seed, mis=n, **more))

    def done(self):
        return Scenario(self.name, self.k, self.s, self.r, self.identity, self.second, self.contigs, self.reads, self.expect)


def ramp_reads(B):
    k, s, ctg = B.k, B.s, B.contigs
    for w in FIRST_WINDOWS:                         # the first window that can seed, for every first chunk of RAMPS
        for direct in "FR":
            B.put("ramp", MAIN, 300 + w, w + k + s + 7, direct, seed=w, first_window=w)
    # two seeds in one chunk: windows 0 .. 3 lie on DUP1, windows from k + s + 4 on lie on MAIN; the lower lane wins
    read = ctg[DUP1][20:20 + k + s + 3] + ctg[MAIN][700:760]
    B.add(read, "two_seeds", **B.intent(read, DUP1, 20, "F", 0))
    # the partner of window 0 is missing (one substitution at k + s - 1): the next pair of clean windows seeds
    broken = [i for i in range(3 * (k + s)) if i <= k + s - 1 < i + k]
    seed = next(i for i in range(3 * (k + s)) if i not in broken and i + s not in broken)
    assert (k, s) != (31, 5) or seed == 36
    read = B.aligned(MAIN, 900, seed + k + s + 9, "F", extra=[k + s - 1])[0]
    B.add(read, "partner_missing", **B.intent(read, MAIN, 900, "F", seed, mis=1 if k + s - 1 < seed else 0))
    # window 0 is unique, its partner and every window up to 70 - k + 1 lie inside the stretch DUP1 shares with DUP2
    read = B.aligned(DUP1, 199, 70 + s + 30, "F")[0]
    B.add(read, "partner_dup", **B.intent(read, DUP1, 199, "F", 70 - k + 2, mis=0))
    assert ctg[DUP1][200:270] == ctg[DUP2][150:220]
    # window 0 is JOIN_A's, its partner window s is JOIN_B's; from window s on the read follows JOIN_B
    read = ctg[JOIN_A][200 - s:200] + ctg[JOIN_B][200:200 + k + s + 20]
    B.add(read, "partner_other_contig", **B.intent(read, JOIN_B, 200 - s, "F", s))
    if k >= 2 * s:
        # inverted: the partner k-mer lies s BEFORE the first one on the contig (a stretch of period 2s makes both fit one read)
        p = 101 + s
        fwd = ctg[PERIODIC][p:p + k] + ctg[PERIODIC][p + k - 2 * s:p + k - s]
        assert fwd[s:s + k] == ctg[PERIODIC][p - s:p - s + k]
        for direct, read in (("F", fwd), ("R", rc(fwd))):
            B.add(read, "inverted", seed=0, direct=direct, contig=PERIODIC, left=0, right=0, mis=0, accepted=True, second="none",
                  hit=(PERIODIC, 1, k + s, p + 1, p - s + k, 0, k + s, ord(direct)))


def ext_reads(B):
    """both extension loops at 0, 1, 63, 64, 65 and 129 positions, ended by the read and by the contig, F and R"""
    k, s, C = B.k, B.s, len(B.contigs[MAIN])
    for n in EXT_LENGTHS:
        for side in ("left", "right"):
            for direct in "FR":
                L = n + k + s
                f = n if side == "left" else 0          # start of the seed in the forward read
                B.put("ext_read_end", MAIN, 400, L, direct, seed=f if direct == "F" else L - f - s - k, ext=(side, n), limit="read")
                # five bases of junk hang over the contig's start (left) or end (right)
                a, f = (-5, n + 5) if side == "left" else (C - L, 0)
                B.put("ext_contig_end", MAIN, a, L + 5, direct, seed=f if direct == "F" else L + 5 - f - s - k, ext=(side, n),
                      limit="contig")
    for direct in "FR":                                 # seeds flush with the contig's start and end, the read going on beyond
        B.put("flush", MAIN, -5, 5 + k + s + 6, direct, seed=5 if direct == "F" else 6, flush="start")
        B.put("flush", MAIN, C - 6 - k - s, 6 + k + s + 5, direct, seed=6 if direct == "F" else 5, flush="end")
    for direct in "FR":                                 # F: the rightward loop, R: the leftward one (the seed is the read's window 0)
        B.put("ext_mismatch_stride2", MAIN, 500, k + s + 129, direct, extra=[k + s - 1 + 64, k + s - 1 + 65], offsets=(64, 65))
        for n in (1, 63, 64, 65, 129):
            B.put("ext_mismatch_last", MAIN, 520, k + s + n, direct, extra=[k + s + n - 1], ext=n, limit="read")
        for n in (64, 129):
            a = C - (k + s + n) if direct == "F" else -5
            B.put("ext_mismatch_last", MAIN, a, k + s + n + 5, direct, extra=[k + s + n - 1], ext=n, limit="contig")


def staging_scenario():
    """reads of 1023, 1024, 1025 and 1100 bases that seed in their last window only, each at batch byte offsets 0 .. 3 mod 4"""
    k, s = 31, 5
    B = Builder("staging", k, s, second=True)
    for n in range(4):
        B.skip(B.contigs[MAIN][:n], "tiny", offset_mod4=sum(len(q) for q in B.reads) % 4)
    for L in STAGED:
        for shift in range(4):
            for direct in "FR":
                at = sum(len(q) for q in B.reads)
                pad = (shift - at) % 4
                if pad:
                    B.skip(B.contigs[MAIN][7:7 + pad], "tiny", offset_mod4=at % 4)
                B.put("staging", MAIN, 100 + shift, L, direct, seed=L - k - s, offset_mod4=shift, length=L)
    B.put("staging", MAIN, 50, SLICE, "F", seed=SLICE - k - s, offset_mod4=sum(len(q) for q in B.reads) % 4, length=SLICE, last=True)
    return B.done()


def most_accepted(align_len, identity):
    m = -1
    while m < align_len and MR.accepted(m + 1, align_len, identity):
        m += 1
    return m


def identity_scenario(identity, tag):
    """reads with exactly the largest accepted number of mismatches and with one more"""
    k, s = 31, 5
    B = Builder("identity_" + tag, k, s, identity=identity)
    pair = 0
    for n, A in enumerate((k + s, 100, 267, 299, 300, 333)):
        m = most_accepted(A, identity)
        assert m >= 0
        direct = "FR"[n % 2]
        for mis in (m, m + 1):
            if mis <= A - k - s:
                B.put("identity_edge", MAIN, 600 + n, A, direct, extra=range(A - mis, A), partner=pair)
        pair += 1
    return B.done()


def growth_scenario():
    """two batches through one Mapper: the identity table has to grow, and align_len == the longest read must be looked up"""
    k, s = 31, 5
    B = Builder("accept_growth", k, s, identity=0.97)
    for n, L in enumerate((36, 100, 150, 199, 200)):
        B.put("accept_growth", MAIN, 30 + n, L, "FR"[n % 2], batch=0)
    m = most_accepted(SLICE + 1, 0.97)
    for n, mis in enumerate((0, 0, m, m + 1)):
        B.put("accept_growth", MAIN, 200 + n, SLICE + 1, "FR"[n % 2], extra=range(SLICE + 1 - mis, SLICE + 1), batch=1)
    return B.done()


def second_scenario(second):
    k, s = 31, 5
    B = Builder("second_on" if second else "second_off", k, s, identity=0.97, second=second)
    A, Bc = B.contigs[MAIN], B.contigs[JOIN_B]
    head = A[len(A) - 80:]                              # the first alignment ends with the contig, at read position 80
    on = (lambda cat, state: (cat, state)) if second else (lambda cat, state: ("second_off", "none"))

    def put(read, cat, state, a, direct, seed, cid=MAIN, **more):
        cat, state = on(cat, state)
        B.add(read, cat, **dict(B.intent(read, cid, a, direct, seed, **more), second=state))

    put(head + Bc[:k + s - 1], "second_gate", "none", len(A) - 80, "F", 0, rest=k + s - 1)
    put(head + Bc[:k + s], "second_gate", "hit", len(A) - 80, "F", 0, rest=k + s)
    # the same read reversed: the first alignment is JOIN_B's k + s bases, the rest of 80 bases is scanned and found on MAIN
    put(rc(head + Bc[:k + s]), "second_gate", "hit", -80, "R", 0, cid=JOIN_B, rest=80)
    bad = bytearray(A[len(A) - 120:])
    for p in range(0, 60, 10):
        bad[p] = other(bad[p])
    put(bytes(bad) + Bc[:k + s], "second_first_rejected", "none", len(A) - 120, "F", 51, mis=6)
    # a second seed in the middle of JOIN_B: its leftward extension runs over the 80 bases of MAIN and is rejected
    put(head + Bc[100:100 + k + s + 20], "second_rejected", "rejected", len(A) - 80, "F", 0)
    return B.done()


def length_reads(B):
    k, s = B.k, B.s
    for d in (-1, 0, 1):
        for direct in "FR":
            if d < 0:
                B.skip(B.aligned(MAIN, 800, k + s + d, direct)[0], "length_edge", length=d)
            else:
                B.put("length_edge", MAIN, 800, k + s + d, direct, length=d)
            B.skip(b"", "empty")


def below_r_scenario(k, s):
    r = k + s + 20
    B = Builder("below_r_k%ds%d" % (k, s), k, s, r=r)
    for direct in "FR":
        B.skip(B.aligned(MAIN, 850, r - 1, direct)[0], "below_r", length=r - 1)
        B.put("below_r", MAIN, 850, r, direct, length=r)
    return B.done()


def find(ok, lo=0, hi=1400):
    return next(a for a in range(lo, hi) if ok(a))


def letter_reads(B, odd, name):
    """lower case, N, the all-A window and bytes outside ACGTacgtNn.  Code 4 of such a byte is OR-ed in unmasked: it reads as A
    and sets the low bit of the base in front of it.  In the first position of a window the bit lands above the k-mer, so the
    reverse complement is picked: the window is still found where the contig's k-mer is stored as its reverse complement."""
    k, s = B.k, B.s
    M, L = B.contigs[MAIN], 2 * k + s + 10
    cat = (lambda c: "high_bytes") if name == "high" else (lambda c: c)
    if name == "letters":
        for direct in "FR":
            read = B.aligned(MAIN, 300, L, direct)[0]
            B.add(read.lower(), "lower_case", **B.intent(read.lower(), MAIN, 300, direct, 0, mis=L - k - s if direct == "F" else 0))
            for inside in (True, False):             # an A of the read becomes N: the same code, another byte
                p = find(lambda p: read[p] == ord("A"), *((2, k) if inside else (k + s + 2, L)))
                rn = bytearray(read)
                rn[p] = ord("N")
                B.add(rn, "N", **B.intent(rn, MAIN, 300, direct, 0, mis=0 if inside else 1, inside=inside))
        P = B.contigs[POLYA]
        fwd = P[151:151 + k + s + 10]
        B.add(fwd, "key0", **B.intent(fwd, POLYA, 151, "F", 0, mis=0))
        fwd = P[151 - s - 10:151 + k]
        B.add(rc(fwd), "key0", **B.intent(rc(fwd), POLYA, 151 - s - 10, "R", 0, mis=0))
    for byte in odd:
        for direct in "FR":
            def target(a):
                return M[a:a + L] if direct == "F" else rc(M[a:a + L])

            def place(a, p, seed, mis, c, **more):
                read = bytearray(target(a))
                read[p] = byte
                B.add(read, cat(c), **B.intent(read, MAIN, a, direct, seed, mis=mis, byte=byte, **more))

            def stored_rc(w):                        # the canonical k-mer of window w is its reverse complement
                return w > rc(w)
            # first position of window 0, the read's byte there being A
            a = find(lambda a: target(a)[0] == ord("A") and stored_rc(target(a)[:k]))
            place(a, 0, 0, 0, "other_first", found=True)
            a = find(lambda a: target(a)[0] == ord("A") and not stored_rc(target(a)[:k]))
            place(a, 0, 1, 1, "other_first", found=False)
            # last position of window 0: after C or T the bit changes nothing, after A or G windows 0 .. k - 2 change, and
            # window k - 1 (which has the byte in front) is lost where its k-mer is stored forward
            a = find(lambda a: target(a)[k - 1] == ord("A") and target(a)[k - 2] in b"CT")
            place(a, k - 1, 0, 0, "other_last", found=True)
            a = find(lambda a: target(a)[k - 1] == ord("A") and target(a)[k - 2] in b"AG" and not stored_rc(target(a)[k - 1:2 * k - 1]))
            place(a, k - 1, k, 1, "other_last", found=False)
            # only in the extension: one mismatch, forward as it is and reversed through the complement table (-> N)
            place(440, k + s + 3, 0, 1, "other_ext")


def k2_scenario():
    """k = 2, s = 1: ten canonical k-mers in all; AACTG holds four of them once each"""
    B = Builder("k2s1", 2, 1, contigs=[b"AACTG"])
    for a, L in ((0, 3), (0, 4), (0, 5), (1, 3), (1, 4), (2, 3)):
        for direct in "FR":
            B.put("k2", 0, a, L, direct, junk=ord("G"))
    for direct in "FR":                              # G in front and GG behind: GA and GG are no k-mers of the contig
        B.put("k2", 0, -1, 8, direct, seed=1 if direct == "F" else 2, junk=ord("G"))
    return B.done()


@functools.lru_cache(maxsize=None)
def scenarios():
    out = []
    for k, s in GOLDEN_PARAMS:
        B, H = Builder("edges_k%ds%d" % (k, s), k, s), Builder("high_k%ds%d" % (k, s), k, s)
        ramp_reads(B)
        ext_reads(B)
        length_reads(B)
        letter_reads(B, b"-R", "letters")
        letter_reads(H, b"\x80\xff", "high")
        out += [B.done(), H.done()] + [below_r_scenario(k, s)] * ((k, s) in ((31, 5), (15, 40)))
    out += [staging_scenario(), identity_scenario(0.97, "097"), identity_scenario(0.9, "09"), identity_scenario(1.0, "1"),
            growth_scenario(), second_scenario(True), second_scenario(False), k2_scenario()]
    assert len({q.name for q in out}) == len(out)
    for scn in out:
        restated(scn.name, scn)
    return tuple(out)


_RESTATED = {}


def params_of(scn):
    return MR.Params(k=scn.k, s=scn.s, l=0, r=scn.r, i=scn.identity, fmt=2)


def restated(name, scn=None):
    """-> (index, [(h1, h2) of the restatement per read]) of a scenario, computed once.  Asserts the exclusion: no seed with
    contig_end < 1 or contig_start - 1 > len(contig) -- the reference reads out of bounds there and the kernel's clamp is its own"""
    if name not in _RESTATED:
        scn = scn or next(q for q in scenarios() if q.name == name)
        X, P = MR.Index(scn.contigs, scn.k), params_of(scn)
        hits = []
        for read in scn.reads:
            h1, h2 = MR.map_read(X, read, P, scn.second)
            starts = [1] * (len(read) >= max(P.r, scn.k + scn.s)) + [h1.read_end + 1] * (h2 != MR.NO_HIT)
            for start in starts:
                seed = MR.get_align_seed(X, read, start, P)
                assert seed is None or (seed[2] >= 1 and seed[1] - 1 <= len(X.contigs[seed[0]])), (name, seed)
            hits.append((h1, h2))
        _RESTATED[name] = (X, hits)
    return _RESTATED[name]


def census(scn, reads=None):
    """what batch_stats() must count for the reads of a scenario"""
    reads = scn.reads if reads is None else reads
    short = sum(len(q) < max(scn.r, scn.k + scn.s) for q in reads)
    long_ = sum(len(q) > SLICE and len(q) >= max(scn.r, scn.k + scn.s) for q in reads)
    return {"by_lds": len(reads) - short - long_, "by_long": long_, "skipped": short}


def batches(scn):
    """-> [indices of the reads of one batch]"""
    if any("batch" in e for e in scn.expect):
        return [[n for n, e in enumerate(scn.expect) if e["batch"] == b] for b in (0, 1)]
    return [list(range(len(scn.reads)))]


def grid_reads(n_reads):
    """(scenario, indices): n_reads short reads cycling through a dozen of edges_k31s5, for the grid-stride loop"""
    scn = next(q for q in scenarios() if q.name == "edges_k31s5")
    dozen = [n for n, q in enumerate(scn.reads) if len(q) <= 120 and scn.expect[n]["cat"].startswith("ext")][:12]
    assert len(dozen) == 12
    return scn, [dozen[n % 12] for n in range(n_reads)]


def golden_scenarios():
    """what the real reference is run on: its four (k, s), no bytes from 128 on (second_off has the reads of second_on)"""
    return [q for q in scenarios() if (q.k, q.s) in GOLDEN_PARAMS and q.name != "second_off"
            and not any(c >= 128 for r in q.reads for c in r)]
