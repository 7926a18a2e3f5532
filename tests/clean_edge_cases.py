"""Crafted cases for the CLEAN kernels (csrc/dbgk_clean.h): reads that sit on the boundaries the kernels' own structure creates --
the rounds of 64 diagonals, the per-lane fold with its three-key tie rule, the three wave reductions, the loop range trimmed
per round, the 1040-byte LDS slice with its dword staging and sentinel, the switch of form at 1024 read bases and at 4096
adapter bytes; for k_clean_lowqual the last ulp of the running sum, the break and block rules, the 8192-byte chunks staged from
`g_lo & ~3` and the workgroups of 256 reads.  Pure Python, fixed content, no GPU and no library load.

scenarios() returns AdapterScenario (name, adapters [(id, bytes)], cutoff, reads [bytes] in batch order, expect, fill) and
LowqualScenario (name, cutoff, shift, reads [(bases, quals)], expect) tuples.  `fill` is the number of all-N contaminants at the
end of the set that only make it larger than the LDS form holds.  `expect` holds one dict per read with the properties the read
was BUILT to have:

    cat        the category the read belongs to (CATEGORIES lists them all)
    hit        the six fields of dbgk_adapter_hit (NO_HIT: none); or, where the adapter side is not what the read is about,
    score, read   the score and (read_start, read_end) alone
    cells      every (read_end, adapter_end) that holds the maximum against the adapter hit, in row-major order
    lanes      [(lane, round)] of those cells' diagonals;  lane, round: of the winner
    form       "lds" / "global": the kernel form that takes the read
    n, A, t    (rounds) read_len + adapter_len - 1, adapter length, index of the winning diagonal
    length, offset_mod4, last   (staging) read length, byte offset in the batch mod 4, the batch's last read
    block      (start, length, trimmed) of dbgk_lowqual_block;  breaks: the 0-based break points
    edge       (chunks) "last" / "first": the break point is the last byte of a staged chunk / the first of the next
    wg_first_mod4, index   (chunks, groups) what the scenario is counted by

A scenario whose name carries `_unpinned` is restatement-only: the reference indexes outside alphabet[] / Qual2Err with its
bytes.  tests/test_clean_edges_cpu.py checks that the restatement (tests/clean_restatement.py) finds exactly what is stated
here; tests/clean_edges_gpu_steps.py holds the kernels to the restatement."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restatement as CR  # noqa: E402

AdapterScenario = namedtuple("AdapterScenario", "name adapters cutoff reads expect fill")
LowqualScenario = namedtuple("LowqualScenario", "name cutoff shift reads expect")

ADAPTER_CATEGORIES = ["rounds", "tie_same_lane_same_end", "tie_same_lane_earlier_end", "tie_lanes_end", "tie_lanes_diag", "tie_three",
                      "run_reset", "overhang", "staging", "slice_edge", "set_size", "order", "letters", "waves"]
LOWQUAL_CATEGORIES = ["equal_rate", "breaks", "equal_blocks", "N", "quality_bytes", "chunks", "groups"]
CATEGORIES = ADAPTER_CATEGORIES + LOWQUAL_CATEGORIES
TIE_CATEGORIES = [c for c in ADAPTER_CATEGORIES if c.startswith("tie_")]
UNPINNED_CATEGORIES = {"letters", "quality_bytes"}          # the only categories that may have restatement-only cases

SLICE = 1024                                   # kCleanSlice: the longest read that is aligned out of LDS
SET_BYTES = 4096                               # kCleanAdapterBytes: the largest adapter set held in LDS
CHUNK = 8192                                   # kLowqualChunk
GROUP = 256                                    # kLowqualThreads: reads per workgroup of k_clean_lowqual
ROUND_N = (1, 2, 63, 64, 65, 127, 128, 129, 193)
ROUND_A = (1, 12, 33, 64, 65, 130)
STAGED = (1, 2, 3, 4, 5, 1023, 1024)
SET_SIZES = (4093, 4094, 4095, 4096, 4097)
WAVES = (1, 3, 4, 5)
GROUPS = (1, 255, 256, 257, 513)
TELLING = (254, 255, 256, 512)
HIGH_BYTES = (0xC1, 0xE1, 0xC3, 0xC7, 0xD4, 0xF4)
EQUAL_RATE = {"equal_rate_q30": (0.001, 30, 20), "equal_rate_q20": (0.01, 20, 30), "equal_rate_q10": (0.1, 10, 30)}   # -e, Q, longest n

M = b"ACGTTGCAAGGCTA"                           # 14 bases without a repeat of its own
M2 = b"GATCCGTACTGAAC"
NO_HIT = CR.NO_HIT


def other(c):
    """a base that differs from byte c"""
    return b"CGTA"[b"ACGT".index(bytes([c]).upper())]


def lane_round(read_end, adapter_end, A):
    """the diagonal of a cell is d = read_end - adapter_end; diagonals are numbered from -(A - 1), 64 to a round"""
    t = read_end - adapter_end + A - 1
    return t % 64, t // 64


def round_targets(n):
    """indices of the winning diagonal for n diagonals: lane 0 and lane 63 of every round, the first and the last diagonal, and the
    start of the last (partly filled unless n is a multiple of 64) round"""
    return sorted({t for t in (0, 63, 64, 127, 128, 191, 192, n - 1, (n - 1) // 64 * 64) if 0 <= t < n})


class Adapters:
    def __init__(self, name, adapters, cutoff, fill=0):
        ads = [(i, bytes(s)) for i, s in adapters] + [("fill%d" % n, b"N" * 128) for n in range(fill)]
        self.scn = AdapterScenario(name, ads, cutoff, [], [], fill)
        self.total = sum(len(s) for _, s in ads)

    def add(self, seq, cat, **intent):
        seq = bytes(seq)
        form = "global" if self.total > SET_BYTES or len(seq) > SLICE else "lds"
        self.scn.reads.append(seq)
        self.scn.expect.append(dict(intent, cat=cat, form=form))

    def tie(self, read, cat, adapter, cells, start):
        """cells: the (read_end, adapter_end) that hold the maximum, row-major; the first wins, its run is `start` cells long"""
        A = len(self.scn.adapters[adapter][1])
        re_, ae = cells[0]
        lanes = [lane_round(i, j, A) for i, j in cells]
        self.add(read, cat, hit=(adapter, start, re_ - start + 1, re_, ae - start + 1, ae), cells=list(cells), lanes=lanes,
                 lane=lanes[0][0], round=lanes[0][1])


def round_markers(A):
    """[(adapter position, letter)]: the first and the last position, the second and the middle one where they are others"""
    pos = []
    for j in (0, A - 1, 1, A // 2):
        if j < A and j not in pos:
            pos.append(j)
    return list(zip(pos, b"ACGT"))


def _rounds(A):
    """one cell with cutoff 1: read and adapters are all N but for one letter.  The adapters carry A, C, G, T at the positions of
    round_markers(A); letter x at read position i0 meets its adapter's marker at j0 in the cell (i0, j0) on diagonal i0 - j0,
    behind alignments with the adapters before it that find no positive cell.  j0 = A - 1 gives the diagonals 0 .. L - 1 (the
    first among them), j0 = 0 the diagonals A - 1 .. L + A - 2 (the last among them), the other two what lies between when the
    read is shorter than the adapter"""
    marks = round_markers(A)
    b = Adapters("rounds_A%d" % A, [("at%d" % j, b"N" * j + bytes([c]) + b"N" * (A - 1 - j)) for j, c in marks], 1)
    for n in ROUND_N:
        L = n - A + 1
        if L < 1:
            continue
        for t in round_targets(n):
            reached = 0
            for ad, (j0, c) in enumerate(marks):
                i0 = t - (A - 1) + j0
                if not 0 <= i0 < L:
                    continue
                reached += 1
                b.add(b"N" * i0 + bytes([c]) + b"N" * (L - i0 - 1), "rounds", hit=(ad, 1, i0 + 1, i0 + 1, j0 + 1, j0 + 1), n=n, A=A, t=t,
                      lane=t % 64, round=t // 64, first_diagonal=t == 0, last_diagonal=t == n - 1)
            assert reached, (n, A, t)
    return b.scn


def _tie_sets(fill):
    """the tie scenarios: each against the adapter its ties are built on, so that no other adapter of a set decides; with
    `fill` all-N contaminants behind it the set exceeds 4096 bytes and every read takes the global-memory form"""
    tag = "global" if fill else "lds"
    T1 = M + b"C" * 50 + M
    T3 = M + b"CCC" + M
    LATE = M + b"C" * 70 + M2
    EARLY = M2 + b"C" * 30 + M
    T5 = M + b"C" * 50 + M + b"CCC" + M
    out = []
    b = Adapters("tie_t1_" + tag, [("t1", T1)], 14, fill)
    for p in (0, 9, 24, 25):
        lead = b"G" * p
        e = p + 104
        b.tie(lead + b"T" * 90 + M, "tie_same_lane_same_end", 0, [(e, 14), (e, 78)], 14)
        b.tie(lead + b"T" * 40 + M + b"T" * 50 + M + b"TTT", "tie_same_lane_earlier_end", 0,
              [(p + 54, 14), (p + 54, 78), (p + 118, 14), (p + 118, 78)], 14)
    out.append(b.scn)
    b = Adapters("tie_late_" + tag, [("late", LATE)], 14, fill)
    for p in (0, 9, 24, 25):
        b.tie(b"G" * p + b"T" * 40 + M + b"T" * 6 + M2 + b"TTT", "tie_same_lane_earlier_end", 0, [(p + 54, 14), (p + 74, 98)], 14)
    out.append(b.scn)
    b = Adapters("tie_early_" + tag, [("early", EARLY)], 14, fill)
    for p in (0, 9, 24, 25):
        b.tie(b"G" * p + b"T" * 40 + M + b"T" * 6 + M2 + b"TTT", "tie_same_lane_earlier_end", 0, [(p + 54, 58), (p + 74, 14)], 14)
    out.append(b.scn)
    b = Adapters("tie_t3_" + tag, [("t3", T3)], 14, fill)
    for p in (0, 9, 24, 25):
        b.tie(b"G" * p + b"T" * 40 + M + b"T" * 5 + M + b"TTT", "tie_lanes_end", 0,
              [(p + 54, 14), (p + 54, 31), (p + 73, 14), (p + 73, 31)], 14)
        b.tie(b"G" * p + b"T" * 60 + M, "tie_lanes_diag", 0, [(p + 74, 14), (p + 74, 31)], 14)
    out.append(b.scn)
    b = Adapters("tie_t5_" + tag, [("t5", T5)], 14, fill)
    for p in (0, 9, 24, 25):
        e = p + 104
        b.tie(b"G" * p + b"T" * 90 + M, "tie_three", 0, [(e, 14), (e, 78), (e, 95)], 14)
    out.append(b.scn)
    return out


def _run_reset():
    b = Adapters("run_reset", [("m", M)], 5)
    lead = b"T" * 20
    # two matches, a mismatch: the sum falls to exactly 0; the run behind it wins
    b.add(lead + M[:2] + bytes([other(M[2])]) + M[3:] + b"TT", "run_reset", hit=(0, 11, 24, 34, 4, 14), how="to_zero")
    # one match, a mismatch: the sum falls below 0
    b.add(lead + M[:1] + bytes([other(M[1])]) + M[2:] + b"TT", "run_reset", hit=(0, 12, 23, 34, 3, 14), how="below_zero")
    # 4 - 2 + 4: the run survives the mismatch; the next cell is a mismatch
    b.add(lead + M[:4] + bytes([other(M[4])]) + M[5:9] + bytes([other(M[9])]) + b"TT", "run_reset", hit=(0, 6, 21, 29, 1, 9),
          how="survives")
    # 5, three mismatches (the run ends), 5 again: one diagonal reaches its maximum in two runs, the first is reported
    gap = b"CAT"                                # against GCA
    b.add(lead + M[:5] + gap + M[8:13] + bytes([other(M[13])]) + b"T", "run_reset", hit=(0, 5, 21, 25, 1, 5), how="twice_two_runs",
          cells=[(25, 5), (33, 13)])
    # 5, two mismatches (5 - 4 = 1: the run goes on), 4 matches: 5 again in the same run; the first cell is reported
    gap = bytes(other(c) for c in M[5:7])
    b.add(lead + M[:5] + gap + M[7:11] + bytes([other(M[11])]) + b"T", "run_reset", hit=(0, 5, 21, 25, 1, 5), how="twice_one_run",
          cells=[(25, 5), (31, 11)])
    return b.scn


def long_adapter():
    rng = np.random.default_rng(130)
    return bytes(b"ACGT"[v] for v in rng.integers(0, 4, 130))


def _overhang():
    long130 = long_adapter()
    b = Adapters("overhang", [("m", M), ("long130", long130)], 8)
    b.add(M[5:] + b"T" * 30, "overhang", hit=(0, 9, 1, 9, 6, 14), how="read_start")
    b.add(b"T" * 50 + M[:9], "overhang", hit=(0, 9, 51, 59, 1, 9), how="read_end")
    b.add(long130[40:60], "overhang", hit=(1, 20, 1, 20, 41, 60), how="adapter_longer")
    b.add(long130[110:], "overhang", hit=(1, 20, 1, 20, 111, 130), how="adapter_longer")
    b.add(long130[:20], "overhang", hit=(1, 20, 1, 20, 1, 20), how="adapter_longer")
    return b.scn


def _tiny():
    b = Adapters("tiny", [("a", b"A")], 1)                    # a set of one adapter of one base
    b.add(b"A", "overhang", hit=(0, 1, 1, 1, 1, 1), how="one_by_one")
    b.add(b"C", "overhang", hit=NO_HIT, how="one_by_one")
    b.add(b"a", "overhang", hit=(0, 1, 1, 1, 1, 1), how="one_by_one")
    b.add(b"", "order", hit=NO_HIT, how="empty_read")
    b.add(b"CA", "order", hit=(0, 1, 2, 2, 1, 1), how="single_adapter")
    return b.scn


def _staging():
    """every staged length at every byte offset mod 4.  A short read is M[5:5 + L]; the read before it ends with M[:5] and the
    read behind it begins with the rest of M, so a byte taken from either neighbour raises the score above L.  A long read
    begins with M[5:] and ends with M[:9]: 9 twice, the first wins, and a neighbour's byte on either side would make 14"""
    b = Adapters("staging", [("m", M)], 1)
    order = [(L, o) for L in STAGED for o in range(4) if (L, o) != (SLICE, 3)] + [(SLICE, 3)]
    at, rest = 0, b""
    for n, (L, o) in enumerate(order):
        q = (o - (at + len(rest) + 5)) % 4
        pad = rest + b"C" * q + M[:5]
        b.add(pad, "staging", pad=True, length=len(pad), offset_mod4=at % 4, last=False)
        at += len(pad)
        last = n == len(order) - 1
        if L <= 5:
            read, rest = M[5:5 + L], M[5 + L:]
            b.add(read, "staging", score=L, read=(1, L), length=L, offset_mod4=at % 4, last=last, pad=False)
        else:
            read, rest = M[5:] + b"C" * (L - 18) + M[:9], M[9:]
            b.add(read, "staging", hit=(0, 9, 1, 9, 6, 14), cells=[(9, 14), (L, 9)], length=L, offset_mod4=at % 4, last=last, pad=False)
        at += L
    return b.scn


def _slice_edge():
    b = Adapters("slice_edge", [("m", M)], 12)
    for L in (SLICE, SLICE + 1, 1100):
        b.add(b"C" * (L - 17) + M + b"TTT", "slice_edge", hit=(0, 14, L - 16, L - 3, 1, 14), length=L)
    return b.scn


def _set_size(total):
    """31 contaminants of 130 N and a last one that brings the set to `total` bytes; its last 14 bases, the set's last bytes, are M"""
    k = total - 31 * 130 - 14
    ads = [("n%d" % n, b"N" * 130) for n in range(31)] + [("last", b"C" * k + M)]
    b = Adapters("set_size_%d" % total, ads, 12)
    b.add(b"T" * 30 + M + b"TT", "set_size", hit=(31, 14, 31, 44, k + 1, k + 14), total=total)
    b.add(b"T" * 30 + M, "set_size", hit=(31, 14, 31, 44, k + 1, k + 14), total=total)          # the read ends with the set
    b.add(b"T" * 30 + M[:11] + b"TT", "set_size", hit=NO_HIT, total=total)
    return b.scn


def _order():
    b = Adapters("order", [("short", M[:8]), ("empty", b""), ("full", M)], 8)
    lead = b"T" * 30
    b.add(lead + M + b"TT", "order", hit=(0, 8, 31, 38, 1, 8), how="first_to_reach", later_score=14)
    b.add(lead + M[:8] + bytes([other(M[8])]) + b"TT", "order", hit=(0, 8, 31, 38, 1, 8), how="equal_cutoff")
    b.add(lead + M[:7] + bytes([other(M[7])]) + b"TT", "order", hit=NO_HIT, how="below_cutoff", best=7)
    b.add(lead[:-1] + b"C" + M[4:] + b"TT", "order", hit=(2, 10, 31, 40, 5, 14), how="behind_empty")
    b.add(b"", "order", hit=NO_HIT, how="empty_read")
    b.add(lead[:-1] + b"C" + M[5:] + b"TT", "order", hit=(2, 9, 31, 39, 6, 14), how="behind_empty")
    return b.scn


def _letters():
    """7 - 2 + 6 = 11 wherever one position of M does not count as a match; 14 where it does"""
    def sub(s, c):
        return s[:7] + c + s[8:]
    b = Adapters("letters", [("withN", sub(M, b"N")), ("withR", sub(M2, b"R"))], 8)
    lead = b"T" * 20
    split = (11, 21, 34, 1, 14)
    b.add(lead + sub(M, b"N") + b"T", "letters", hit=(0,) + split, how="N_N")
    b.add(lead + sub(M, b"n") + b"T", "letters", hit=(0,) + split, how="n_N")
    b.add(lead + M + b"T", "letters", hit=(0,) + split, how="base_N")
    b.add(lead + M.lower() + b"T", "letters", hit=(0,) + split, how="lower_read")
    b.add(lead + sub(M2, b"R") + b"T", "letters", hit=(1,) + split, how="R_R")
    b.add(lead + M2 + b"T", "letters", hit=(1,) + split, how="base_R")
    for c in b"-.*":
        b.add(lead + sub(M2, bytes([c])) + b"T", "letters", hit=(1,) + split, how="other_byte", byte=c)
    return b.scn


def _letters_lower():
    b = Adapters("letters_lower", [("lower", M.lower()), ("withY", M2[:7] + b"Y" + M2[8:])], 8)
    lead = b"T" * 20
    b.add(lead + M + b"T", "letters", hit=(0, 14, 21, 34, 1, 14), how="lower_adapter")
    b.add(lead + M.lower() + b"T", "letters", hit=(0, 14, 21, 34, 1, 14), how="lower_both")
    b.add(lead + M2[:7] + b"Y" + M2[8:] + b"T", "letters", hit=(1, 11, 21, 34, 1, 14), how="Y_Y")
    b.add(lead + M2[:7] + b"y" + M2[8:] + b"T", "letters", hit=(1, 11, 21, 34, 1, 14), how="y_Y")
    return b.scn


def _letters_high():
    """bytes that equal a letter in their low seven bits: reachable through the C ABI only"""
    out = []
    b = Adapters("letters_high_read_unpinned", [("m", M)], 8)
    lead = b"T" * 20
    for c in HIGH_BYTES:
        p = M.index(bytes([c & 0x5F]), 3)                 # behind the first bases: p - 2 + (13 - p) = 11 beats either side alone
        assert 3 <= p <= 10
        b.add(lead + M[:p] + bytes([c]) + M[p + 1:] + b"T", "letters", hit=(0, 11, 21, 34, 1, 14), how="high_byte", byte=c)
    out.append(b.scn)
    b = Adapters("letters_high_adapter_unpinned", [("high", M[:7] + b"\xC1" + M[8:]), ("high2", M2[:4] + b"\xC3" + M2[5:])], 8)
    b.add(lead + M + b"T", "letters", hit=(0, 11, 21, 34, 1, 14), how="high_byte", byte=0xC1)
    b.add(lead + M[:7] + b"\xC1" + M[8:] + b"T", "letters", hit=(0, 11, 21, 34, 1, 14), how="high_byte", byte=0xC1)
    b.add(lead + M2 + b"T", "letters", hit=(1, 11, 21, 34, 1, 14), how="high_byte", byte=0xC3)
    out.append(b.scn)
    return out


def _waves(n):
    b = Adapters("waves_%d" % n, [("m", M)], 12)
    for r in range(n - 1):
        b.add(b"T" * (30 + r) + M[:11] + b"TT", "waves", hit=NO_HIT, batch=n)
    b.add(b"T" * 30 + M + b"TT", "waves", hit=(0, 14, 31, 44, 1, 14), batch=n)
    return b.scn


# ---- k_clean_lowqual --------------------------------------------------------------------------------------------------------------

class Lowqual:
    def __init__(self, name, cutoff=0.001, shift=33):
        self.scn = LowqualScenario(name, cutoff, shift, [], [])
        self.hi, self.lo = bytes([shift + 40]), bytes([shift + 2])       # Q40: 1e-4; Q2: 0.63

    def add(self, bases, quals, cat, **intent):
        assert len(bases) == len(quals)
        self.scn.reads.append((bytes(bases), bytes(quals)))
        self.scn.expect.append(dict(intent, cat=cat))

    def q(self, pattern):
        """'I' -> Q40, '#' -> Q2"""
        return b"".join(self.hi if c == "I" else self.lo for c in pattern)

    def plain(self, pattern, cat, block, **intent):
        self.add(b"A" * len(pattern), self.q(pattern), cat, block=block, breaks=[j for j, c in enumerate(pattern) if c == "#"], **intent)

    def bytes_at(self):
        return sum(len(b) for b, _ in self.scn.reads)


def equal_rate_trimmed(name, n):
    """what the issue found with the restatement and this libm: the decision is the last ulp of the running sum"""
    return {"equal_rate_q30": n >= 10, "equal_rate_q20": n == 6 or n >= 18, "equal_rate_q10": n >= 15}[name]


def _equal_rate(name):
    cutoff, Q, top = EQUAL_RATE[name]
    b = Lowqual(name, cutoff, 33)
    for n in range(1, top + 1):
        b.add(b"A" * n, bytes([33 + Q]) * n, "equal_rate", trimmed=equal_rate_trimmed(name, n), length=n)
    return b.scn


def _blocks():
    b = Lowqual("blocks")
    b.plain("#" * 10, "breaks", (0, 0, 1), how="every_base")
    b.plain("#", "breaks", (0, 0, 1), how="every_base")
    b.plain("#" + "I" * 11, "breaks", (2, 11, 1), how="first_only")
    b.plain("I" * 11 + "#", "breaks", (1, 11, 1), how="last_only")
    b.plain("I" * 12, "breaks", (1, 12, 0), how="not_trimmed")
    b.scn.expect[-1]["breaks"] = None
    b.add(b"", b"", "breaks", block=(0, 0, 0), breaks=None, how="empty")
    b.plain("I" * 10 + "#" + "I" * 10 + "#" + "I" * 5, "equal_blocks", (1, 10, 1), how="two_equal")
    b.plain("I" * 10 + "#" + "I" * 10 + "#" + "I" * 10 + "#" + "I" * 3, "equal_blocks", (1, 10, 1), how="three_equal")
    b.plain("I" * 10 + "#" + "I" * 11 + "#" + "I" * 3, "equal_blocks", (12, 11, 1), how="later_longer")
    b.plain("I" * 10 + "#" + "I" * 10, "equal_blocks", (1, 10, 1), how="tail_equal")
    b.plain("I" * 10 + "#" + "I" * 11, "equal_blocks", (12, 11, 1), how="tail_longer")
    return b.scn


def _N(shift):
    b = Lowqual("N_shift%d" % shift, 0.001, shift)
    b.add(b"AAAAANAAAA", b.hi * 10, "N", block=(1, 5, 1), breaks=[5], how="N", shift=shift)
    b.add(b"AAAAAnAAAA", b.hi * 10, "N", block=(1, 10, 0), breaks=None, how="n", shift=shift)
    b.add(b"NAAAAAAAAA", b.hi * 10, "N", block=(2, 9, 1), breaks=[0], how="N", shift=shift)
    b.add(b"AAAAAAAAAN", b.hi * 9 + b.lo, "N", block=(1, 9, 1), breaks=[9], how="N", shift=shift)
    return b.scn


def _quality_bytes():
    """shift 20, so that shift + 99 = 119 is a byte: Q99 = 1.26e-10 breaks at -e 1e-12, the bytes 120..127 behind the table's last
    entry hold no error, nor does a byte below the shift"""
    b = Lowqual("quality_bytes_shift20", 1e-12, 20)
    q = bytes([119] + list(range(120, 128)) + [119])
    b.add(b"A" * 10, q, "quality_bytes", block=(2, 8, 1), breaks=[0, 9], how="table_end")
    b.add(b"A" * 4, bytes([19, 15, 0x0B, 19]), "quality_bytes", block=(1, 4, 0), breaks=None, how="below_shift")
    b.add(b"A" * 5, bytes([19, 19, 20, 19, 19]), "quality_bytes", block=(1, 2, 1), breaks=[2], how="below_shift")     # Q0 = 1.0
    return b.scn


def _quality_high():
    b = Lowqual("quality_bytes_high_unpinned")
    b.add(b"A" * 7, b.hi * 3 + bytes([128, 200, 255]) + b.lo, "quality_bytes", block=(1, 6, 1), breaks=[6], how="high")
    b.add(b"A" * 3, bytes([128, 161, 255]), "quality_bytes", block=(1, 3, 0), breaks=None, how="high")
    b.add(b"AA\xCEAA", b.hi * 5, "quality_bytes", block=(1, 5, 0), breaks=None, how="high_base")      # 0xCE is 'N' + 128: not an N
    return b.scn


def _chunks():
    """six workgroups of 256 reads.  The first four begin at byte offset mod 4 = 0, 1, 2, 3 and each holds a read whose only break
    point is the last byte of the workgroup's first staged chunk and one whose only break point is the first byte of its third;
    the first also has reads of 8192, 8193 and 16 500 bases; the fifth is all empty reads, the sixth has a few reads"""
    b = Lowqual("chunks", 0.000101)             # Q40 = 1e-4 never breaks, and one Q2 base trims a read of any length here
    fillers = ("I", "#I", "II#", "I" * 5)
    blocks = {"I": (1, 1, 0), "#I": (2, 1, 1), "II#": (1, 2, 1), "IIIII": (1, 5, 0)}
    for wg in range(4):
        start = b.bytes_at()
        assert start % 4 == wg
        base = start & ~3
        count0 = len(b.scn.reads)
        if wg:
            b.add(b"", b"", "chunks", block=(0, 0, 0), breaks=None, how="empty_first", wg_first_mod4=wg)
        for edge, pos in (("last", base + CHUNK - 1), ("first", base + 2 * CHUNK)):
            at = b.bytes_at()
            idx = pos - at
            assert 50 < idx < 8300 - 50
            pattern = "I" * idx + "#" + "I" * (8300 - idx - 1)
            b.plain(pattern, "chunks", (1, idx, 1) if idx >= 8300 - idx - 1 else (idx + 2, 8300 - idx - 1, 1), how="straddle", edge=edge,
                    at=pos - base, wg_first_mod4=wg)
        if wg == 0:
            for n in (CHUNK, CHUNK + 1, 16500):
                b.plain("I" * (n - 1) + "#", "chunks", (1, n - 1, 1), how="long", length=n, wg_first_mod4=wg)
        n_fill = GROUP - (len(b.scn.reads) - count0) - (1 if wg else 0)
        for n in range(n_fill):
            p = fillers[n % len(fillers)]
            if n == n_fill - 1:                              # the workgroup behind begins at offset mod 4 = wg + 1
                p = "I" * (1 + (wg + 1 - (b.bytes_at() + 1)) % 4)
                b.plain(p, "chunks", (1, len(p), 0), how="fill", wg_first_mod4=wg)
                b.scn.expect[-1]["breaks"] = None
                continue
            b.plain(p, "chunks", blocks[p], how="fill", wg_first_mod4=wg)
            if not blocks[p][2]:
                b.scn.expect[-1]["breaks"] = None
        if wg:
            b.add(b"", b"", "chunks", block=(0, 0, 0), breaks=None, how="empty_last", wg_first_mod4=wg)
        assert len(b.scn.reads) - count0 == GROUP
    for n in range(GROUP):
        b.add(b"", b"", "chunks", block=(0, 0, 0), breaks=None, how="empty_group")
    for p in ("II#", "#I", "I" * 9 + "#" + "I" * 9):
        b.plain(p, "chunks", {"II#": (1, 2, 1), "#I": (2, 1, 1)}.get(p, (1, 9, 1)), how="behind_empty_group")
    return b.scn


def _groups(size):
    b = Lowqual("groups_%d" % size)
    for n in range(size):
        if n in TELLING or (size == 1 and n == 0):
            k = 2 + n % 3
            b.plain("I" * k + "#" + "I", "groups", (1, k, 1), index=n, batch=size, telling=True)
        else:
            b.plain("III", "groups", (1, 3, 0), index=n, batch=size, telling=False)
            b.scn.expect[-1]["breaks"] = None
    return b.scn


@functools.lru_cache(maxsize=None)
def scenarios():
    out = [_rounds(A) for A in ROUND_A]
    out += _tie_sets(0) + _tie_sets(33)
    out += [_run_reset(), _overhang(), _tiny(), _staging(), _slice_edge()]
    out += [_set_size(t) for t in SET_SIZES]
    out += [_order(), _letters(), _letters_lower()] + _letters_high()
    out += [_waves(n) for n in WAVES]
    out += [_equal_rate(n) for n in EQUAL_RATE]
    out += [_blocks(), _N(33), _N(64), _quality_bytes(), _quality_high(), _chunks()]
    out += [_groups(n) for n in GROUPS]
    assert len({s.name for s in out}) == len(out)
    return tuple(out)


def adapter_scenarios():
    return [s for s in scenarios() if isinstance(s, AdapterScenario)]


def lowqual_scenarios():
    return [s for s in scenarios() if isinstance(s, LowqualScenario)]


def scenario(name):
    return next(s for s in scenarios() if s.name == name)


def pinned(scn):
    return "_unpinned" not in scn.name


def census(scn):
    """what the construction says dbgk_clean_stats must count for an adapter scenario (hits and cells need the restated hits)"""
    return {"reads": len(scn.reads), "by_lds": sum(e["form"] == "lds" for e in scn.expect), "by_global": sum(e["form"] == "global" for e in scn.expect)}


def text(b):
    return bytes(b).decode("latin-1")


def named_adapters(scn):
    return [(i, text(s)) for i, s in scn.adapters]


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's numbers for a scenario: six-field hits, or (error_sum, start, length, trimmed) blocks"""
    scn = scenario(name)
    if isinstance(scn, AdapterScenario):
        return CR.align_many(list(scn.reads), named_adapters(scn), scn.cutoff, cells_per_chunk=1 << 16)
    table = CR.error_table(scn.shift)
    return [CR.lowqual_block(text(b), text(q), scn.cutoff, scn.shift, table) for b, q in scn.reads]


def cells_of(scn, hits):
    """the `cells` counter: read_len * adapter_len of every alignment up to the adapter that is hit"""
    total = 0
    for read, h in zip(scn.reads, hits):
        tried = scn.adapters if h[0] < 0 else scn.adapters[:h[0] + 1]
        total += sum(len(read) * len(s) for _, s in tried)
    return total


def fastq(scn):
    """the scenario as the FASTQ file the two programs read (adapter reads get Q40 throughout)"""
    out = []
    for n, r in enumerate(scn.reads):
        bases, quals = r if isinstance(scn, LowqualScenario) else (r, b"I" * len(r))
        out.append(b"@%s_%d %s\n%s\n+\n%s\n" % (scn.name.encode(), n, scn.expect[n]["cat"].encode(), bases, quals))
    return b"".join(out)


def fasta(scn):
    return b"".join(b">%s\n%s\n" % (i.encode(), s) for i, s in scn.adapters)


def case_of(scn):
    """the command line of a pinned scenario, as tests/golden/clean_edges/cases.json lists it"""
    if isinstance(scn, AdapterScenario):
        return {"name": scn.name, "program": "clean_adapter", "args": ["-a", scn.name + ".fa", "-s", str(scn.cutoff), "-r", "0"],
                "input": scn.name + ".fq.gz"}
    return {"name": scn.name, "program": "clean_lowqual", "args": ["-e", repr(scn.cutoff), "-q", str(scn.shift), "-r", "0"],
            "input": scn.name + ".fq.gz"}
