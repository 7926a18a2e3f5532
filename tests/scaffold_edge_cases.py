"""Crafted cases for the scaffolding stages LINK (csrc/dbgk_link.h) and FILL (csrc/dbgk_fill.h): records that sit on the boundaries
the kernels' own structure creates -- the 64-column work unit of k_fill_consensus and its reversed index, the 64-read rounds of its
spanning-read loop and of the bad-slice pre-check, the end of a read, the gallop and bisection of fill_run_end, the sign order of
the gap sort key, the cap on the consensus launch, the four shapes of link_orient at the two ends of the gap filter, the 1023 cap
across batches, a gap sum beyond 2^31, first-seen order, and the drop conditions for mapper hits.  Pure numpy, fixed seeds, no GPU,
no library load and no reference.

fill_scenarios() returns Fill tuples (name, n, lens, reads, recs, cuts, expect): -n, contig lengths, the reads as latin-1 strings
(a record's `read` field indexes them), FR.REC_DTYPE records in file order, the batch boundaries they are fed at, and `expect`:
what the scenario was BUILT to show.  link_scenarios() returns Link tuples (name, P, lens, recs, cuts, expect) with LR.PAIR_DTYPE
records.  slice_jobs(), fill_hits() and link_hits() hold the jobs that are no plain record list.  tests/test_scaffold_edges_cpu.py
checks that the restatements (tests/fill_restatement.py, tests/link_restatement.py) find exactly what `expect` says, that the naive
restatements below (naive_link_table, naive_gap_stats: record by record, dict of lists, no sort) agree with the vectorised ones, and
that both reproduce what the real reference wrote for the subset stored in tests/golden/scaffold_edges;
tests/scaffold_edges_gpu_steps.py holds the kernels to the restatements.

Every FILL junction is its own pair of contigs (2j, 2j + 1), so every gap appears in the layout.  A forward read is F F on
(c1, c2); a read of the other strand is R R with the contigs exchanged and holds the reverse complement of its columns."""
import functools
import itertools
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import fill_restatement as FR  # noqa: E402
import link_restatement as LR  # noqa: E402
import make_link_golden as MLG  # noqa: E402  (its Scenario solves every class's gap formula for start and end)

if os.path.isdir(MLG.WORK) and not os.listdir(MLG.WORK):
    os.rmdir(MLG.WORK)                          # the maker's scratch directory: not needed for its Scenario class

Fill = namedtuple("Fill", "name n lens reads recs cuts expect")
Link = namedtuple("Link", "name P lens recs cuts expect")

WIDTHS = (1, 63, 64, 65, 127, 128, 129, 200)
SPANS = (1, 2, 63, 64, 65, 128, 129, 200)
GOLDEN_WIDTHS = (63, 64, 65, 129, 200)         # what goes to the real reference (tests/golden/scaffold_edges)
GOLDEN_SPANS = (3, 64, 65)
RUN_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025)
GOLDEN_RUN_LENGTHS = RUN_LENGTHS[:14]          # ... plus one run of 1024
LETTERS = "ACGNT"                              # ascending as map<char,int> iterates them
TIE_COLUMNS = (0, 63, 64, 127, 128, 129)
BAD_AT = (0, 63, 64, 129)                      # spanning index of the offending read: every lane group of the pre-check loop
UNITS_JUNCTIONS = 40000
CAP_COUNTS = (1022, 1023, 1024, 1025, 2047)
BIG_INSERT = 3000000


def rand_bytes(rng, n, alphabet="ACGT"):
    return "".join(alphabet[v] for v in rng.integers(0, len(alphabet), n))


class FillJob:
    """records and reads of a FILL job, junction by junction"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.lens, self.rows, self.reads = [], [], []

    def pair(self):
        c = len(self.lens)
        self.lens += [int(x) for x in self.rng.integers(50, 150, 2)]
        return c, c + 1

    def rec(self, c1, c2, gap, cols=None, other=False, spare=0, lead=None, alphabet="ACGT", d=None):
        """one read over c1 -> c2 that leaves `gap`; cols: the gap's columns as the scafftig reads them (gap > 0), random without;
        other: the read is of the other strand; spare: bytes behind the slice; lead: align1_end, drawn from 0 .. 50 without"""
        lead = int(self.rng.integers(0, 51)) if lead is None else lead
        width = max(gap, 0)
        cols = rand_bytes(self.rng, width, alphabet) if cols is None else cols
        assert len(cols) == width
        body = FR.rev_com_seq(cols) if other else cols
        read = rand_bytes(self.rng, lead) + body + rand_bytes(self.rng, spare if lead + width + spare else 1)   # no empty read
        a, b, d1, d2 = (c2, c1, "R", "R") if other else (c1, c2, "F", "F")
        if d:
            d1, d2 = d
        self.rows.append((len(self.reads), len(read), lead, lead + gap + 1, a, b, ord(d1), ord(d2), (0, 0)))
        self.reads.append(read)

    def done(self, name, n=1, cuts=None, shuffle=None, expect=None):
        recs = np.array(self.rows, dtype=FR.REC_DTYPE)
        reads = self.reads
        if shuffle is not None:
            order = np.random.default_rng(shuffle).permutation(len(recs))
            recs = recs[order]
            reads = [reads[i] for i in recs["read"].tolist()]
            recs["read"] = np.arange(len(recs))  # a read's index is the place of its first record, as the parser numbers them
        return Fill(name, n, list(self.lens), reads, recs, cuts or [0, len(recs)], expect or {})


# ---- FILL -------------------------------------------------------------------------------------------------------------------

def widths_x_spans(widths=WIDTHS, spans=SPANS, name="widths_x_spans"):
    """one junction per (w, s): the mode w with frequency s; forward and other-strand reads alternate, so both strands cross every
    64-column unit and every 64-read round; record 0 of a junction ends with its slice, the others have 0 .. 2 spare bytes; with
    s > 2 two more records of gap w + 1 and w - 1 (w == 1: w + 2), so the mode is a middle (w == 1: the first) run of its pair"""
    J = FillJob(41)
    for w, s in itertools.product(widths, spans):
        c1, c2 = J.pair()
        for k in range(s):
            J.rec(c1, c2, w, other=k % 2 == 1, spare=0 if k == 0 else k % 3, alphabet="ACGTN")
        if s > 2:
            J.rec(c1, c2, w + 1, alphabet="ACGTN")
            J.rec(c1, c2, w - 1 if w > 1 else w + 2, other=True, alphabet="ACGTN")
    n = len(J.rows)
    return J.done(name, cuts=[0, 1, 1, n // 3, n], shuffle=7, expect={"filled": sorted(itertools.product(widths, spans))})


def winner(counts):
    """the byte of the highest count, the smallest byte on a tie: counts in the order of LETTERS"""
    return LETTERS[max(range(5), key=lambda i: (counts[i], -i))]


def tie_gap(J, width, span, widest, pairs, seed):
    """one gap built column by column (counts of A C G N T per column): TIE_COLUMNS hold the patterns of `widest` in turn, the
    other columns run through widest + pairs; the letters of a column are dealt to the reads in a shuffled order; odd reads are
    of the other strand"""
    rng = np.random.default_rng(seed)
    rows = [[None] * width for _ in range(span)]
    counts = []
    cycle = widest + pairs
    for k in range(width):
        p = widest[TIE_COLUMNS.index(k) % len(widest)] if k in TIE_COLUMNS else cycle[k % len(cycle)]
        assert sum(p) == span
        col = [ch for ch, c in zip(LETTERS, p) for _ in range(c)]
        for m, j in enumerate(rng.permutation(span).tolist()):
            rows[m][k] = col[j]
        counts.append(tuple(p))
    c1, c2 = J.pair()
    for m in range(span):
        J.rec(c1, c2, width, cols="".join(rows[m]), other=m % 2 == 1, spare=m % 2)
    return (c1, c2), counts


def tie_patterns(span):
    """-> the widest ties `span` reads can form, and every tied pair for the maximum with the rest spread below it"""
    if span % 5 == 0:
        widest = [(span // 5,) * 5]
    else:                                          # 12 reads: four-way ties, each letter absent in turn
        widest = [tuple(0 if i == z else span // 4 for i in range(5)) for z in range(5)]
    pairs = []
    top = (span - 2) // 2
    for i, j in itertools.combinations(range(5), 2):
        p = [0] * 5
        p[i] = p[j] = top
        for z in [x for x in range(5) if x not in (i, j)][:span - 2 * top]:
            p[z] += 1
        assert sum(p) == span and max(p[z] for z in range(5) if z not in (i, j)) < top
        pairs.append(tuple(p))
    return widest, pairs


def column_ties():
    """two gaps of width 130.  Span 12: every tied pair for the maximum (A=C .. N=T) and four-way ties, each letter absent in turn,
    in TIE_COLUMNS and others -- twelve reads cannot tie five letters.  Span 10: the same pairs and the five-way tie (2 2 2 2 2) in
    TIE_COLUMNS and others.  Half the reads are reversed, so a column's counts come through link_complement."""
    J = FillJob(42)
    expect = {"gaps": {}}
    for span, seed in ((12, 1), (10, 2)):
        widest, pairs = tie_patterns(span)
        pair, counts = tie_gap(J, 130, span, widest, pairs, seed)
        expect["gaps"][pair] = {"span": span, "counts": counts, "consensus": "".join(winner(c) for c in counts)}
    return J.done("column_ties", expect=expect)


def host_path_late():
    """three gaps of width 129 and span 70, reads m % 3 == 1 reversed.  Gap 0: one lower-case g in column 128 of spanning read 69
    (second round of reads, third unit).  Gap 1: in that column byte 0xC1 (35 forward reads, read 69 among them) ties with A: as a
    signed char it comes first and wins.  Gap 2: its only odd bytes are N: no host path."""
    J = FillJob(43)
    pairs = []
    for g in range(3):
        c1, c2 = J.pair()
        pairs.append((c1, c2))
        truth = rand_bytes(J.rng, 129)
        forward = [m for m in range(70) if m % 3 != 1]
        high = set(forward[-35:])
        for m in range(70):
            cols = truth
            if g == 0 and m == 69:
                cols = truth[:128] + "g"
            elif g == 1:
                cols = truth[:128] + ("\xc1" if m in high else "A")
            elif g == 2 and m % 7 == 0:
                k = (m * 37) % 129
                cols = truth[:k] + "N" + truth[k + 1:]
            J.rec(c1, c2, 129, cols=cols, other=m % 3 == 1, spare=m % 2)
    return J.done("host_path_late", expect={"pairs": pairs, "host_path": [1, 1, 0]})


def naive_gap_stats(recs):
    """decide_gap_size record by record: a dict of gap counts per unordered pair, the ascending walk with strict >, the variance in
    wrapping int arithmetic -> {(lo, hi): (mode, mode_freq, total_freq, variance)}"""
    count = {}
    for r in recs.tolist():
        a1e, a2s, c1, c2 = r[2], r[3], r[4], r[5]
        gap = int(FR.wrap32(a2s - a1e - 1))
        d = count.setdefault((min(c1, c2), max(c1, c2)), {})
        d[gap] = d.get(gap, 0) + 1
    out = {}
    for pair, d in count.items():
        mode = freq = 0
        for g in sorted(d):
            if d[g] > freq:
                mode, freq = g, d[g]
        total = sum(d.values())
        var = 0
        for g in sorted(d):
            var = int(FR.wrap32(var + int(FR.wrap32(abs(int(FR.wrap32(g - mode))) * d[g]))))
        out[pair] = (mode, freq, total, LR.c_div(var, total))
    return out


def gapstat_runs(lengths=RUN_LENGTHS, last_single=False, name="gapstat_runs", one_long=None):
    """every pair's gaps are runs of equal value (-40 .. 60).  Per run length L three pairs: the mode (L records) is the first,
    a middle, the last run, the others have L - 1 and L // 2 records (L == 1: a pair of one record).  Then the ties: two-way,
    three-way, {-3 x 4, 2 x 4} (the mode is -3: not filled, the left contig is cut by 3), and one pair whose records come half as
    (c1 < c2) and half as (c1 > c2) with directions that disagree, one of a wrong direction among them.  The first pair holds
    sorted position 0; the last pair ends at n: its last run is its mode, or (last_single) it is a single record."""
    J = FillJob(44)
    runs = {}

    def pair_of(spec, mixed=False):
        """spec: [(gap, count)]"""
        c1, c2 = J.pair()
        k = 0
        for gap, count in spec:
            for _ in range(count):
                if mixed:                              # c1 -> c2 and c2 -> c1 by turns, both F F: the directions disagree
                    a, b = (c1, c2) if k % 2 == 0 else (c2, c1)
                    J.rec(a, b, gap, spare=k % 3, d="FN" if k == 5 else None)
                else:
                    J.rec(c1, c2, gap, other=k % 2 == 1, spare=k % 3)
                k += 1
        runs[(c1, c2)] = spec
        return c1, c2

    for L in lengths:
        for pos in range(3):
            if L == 1:
                if pos == 0:
                    pair_of([(int(J.rng.integers(-40, 61)), 1)])
                continue
            g = sorted(int(x) for x in J.rng.choice(np.arange(-40, 61), 3, replace=False))
            if L >= 1023:
                g = sorted(int(x) for x in J.rng.choice(np.arange(1, 61), 3, replace=False))   # the long runs are filled gaps
            count = [L - 1, max(L // 2, 1)]
            count.insert(pos, L)
            pair_of(list(zip(g, count)))
    if one_long:                                           # (the cut-down job of the goldens: one long run, in the middle)
        pair_of([(6, 3), (14, one_long), (15, 5)])
    pair_of([(5, 4), (9, 4), (11, 3)])                     # two-way: the smaller gap
    pair_of([(-2, 2), (20, 6), (31, 6)])                   # two-way between the middle and the last run
    pair_of([(-6, 3), (7, 3), (8, 3)])                     # three-way
    cut = pair_of([(-3, 4), (2, 4)])                       # negative against positive: sign order of the sort key
    mixed = pair_of([(12, 4), (13, 3)], mixed=True)
    if last_single:
        pair_of([(17, 1)])
    else:
        pair_of([(3, 16), (4, 33), (21, 1025)] if 1025 in lengths else [(3, 16), (4, 32), (21, 33)])
    f = J.done(name, shuffle=9)
    n = len(f.recs)
    return f._replace(cuts=[0, n // 2, n], expect={"stats": naive_gap_stats(f.recs), "runs": runs, "cut": cut, "mixed": mixed})


SliceJob = namedtuple("SliceJob", "name fill refused filled")


@functools.lru_cache(maxsize=None)
def slice_jobs():
    """(a) every spanning read ends exactly with its slice; (b) as (a) with one read of the filled gap of span 130 one byte
    shorter, (c) with align1_end = -1 on one of its records -- the offending read at spanning index 0, 63, 64, 129 in turn;
    (d) every read cut to 5 bytes in a job whose modes are all <= 0: nobody looks at them"""
    def base(name):
        J = FillJob(45)
        c1, c2 = J.pair()
        truth = rand_bytes(J.rng, 70)
        for m in range(130):
            J.rec(c1, c2, 70, cols=truth, other=m % 2 == 1, lead=1 + m % 9)
        c3, c4 = J.pair()
        for m in range(3):
            J.rec(c3, c4, 9, cols=truth[:9], lead=m)
        return J
    out = [SliceJob("exact", base("exact").done("slice_exact"), False, 2)]
    for at in BAD_AT:
        J = base("short")
        J.reads[at] = J.reads[at][:-1]
        out.append(SliceJob("short_%d" % at, J.done("slice_short_%d" % at), True, None))
        J = base("neg")
        r = list(J.rows[at])
        r[2], r[3] = -1, 70                                # align1_end -1, the gap stays 70
        J.rows[at] = tuple(r)
        out.append(SliceJob("negative_%d" % at, J.done("slice_negative_%d" % at), True, None))
    J = FillJob(46)
    for gap in (0, -3, 0, -1, -40):
        c1, c2 = J.pair()
        for m in range(4):
            J.rec(c1, c2, gap, other=m % 2 == 1, lead=40)
        J.rec(c1, c2, 6, lead=40)                          # a positive gap that is not the mode
    J.reads = [r[:5] for r in J.reads]
    out.append(SliceJob("modes_not_positive", J.done("slice_modes_not_positive"), False, 0))
    return out


def more_units_than_waves():
    """40 000 junctions of width 1 .. 3, three records each: one work unit per junction"""
    rng = np.random.default_rng(47)
    nj = UNITS_JUNCTIONS
    width = rng.integers(1, 4, nj)
    lens = rng.integers(50, 150, 2 * nj)
    recs = np.zeros(3 * nj, dtype=FR.REC_DTYPE)
    j = np.repeat(np.arange(nj), 3)
    k = np.tile(np.arange(3), nj)
    other = k == 1
    recs["read"] = np.arange(3 * nj)
    recs["read_len"] = 12
    recs["align1_end"] = 3 + k
    recs["align2_start"] = recs["align1_end"] + width[j] + 1
    recs["contig1"] = np.where(other, 2 * j + 1, 2 * j)
    recs["contig2"] = np.where(other, 2 * j, 2 * j + 1)
    recs["direct1"] = recs["direct2"] = np.where(other, ord("R"), ord("F"))
    arr = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, (3 * nj, 12))]
    reads = [row.tobytes().decode() for row in arr]
    order = rng.permutation(3 * nj)
    recs = recs[order]
    reads = [reads[i] for i in recs["read"].tolist()]
    recs["read"] = np.arange(3 * nj)
    return Fill("more_units_than_waves", 1, lens.tolist(), reads, recs, [0, nj, 3 * nj], {"units": nj, "widths": width})


HIT_DTYPE = np.dtype([("contig", "<i4"), ("read_start", "<i4"), ("read_end", "<i4"), ("contig_start", "<i4"),
                      ("contig_end", "<i4"), ("mismatches", "<i4"), ("align_len", "<i4"), ("direct", "<i4")])   # == capi.MAP_HIT_DTYPE
HIT_KINDS = ("hit1_unmapped", "hit2_unmapped", "same_contig", "contig_is_n", "contig_minus_2", "FF", "RR", "FR", "RF", "wrong")
HitJob = namedtuple("HitJob", "name lens reads hits first_reads kinds kept_rows expect")


def fill_hits():
    """a hand-made hit array [n, 2] for GapFiller.add_hits in two batches (first_read 0 and 7): the drop conditions of
    k_fill_orient<true> beside ordinary reads of all four classes and one wrong direction; kept_rows: the FR.REC_DTYPE records a
    plain filter keeps (map_reads.cpp:59-73 and the range check)"""
    J = FillJob(48)
    n_contigs = 12
    J.lens = [int(x) for x in J.rng.integers(60, 200, n_contigs)]
    kinds, hits, reads, rows = [], [], [], []
    plan = []
    for rep in range(4):
        for kind in HIT_KINDS:
            plan.append(kind)
    plan = [plan[i] for i in np.random.default_rng(5).permutation(len(plan)).tolist()]
    for r, kind in enumerate(plan):
        # FF and RR reads (and the dropped ones) on three junctions: contigs (0, 1), (2, 3), (4, 5) with the gaps 4, 34, 64;
        # FR, RF and wrong reads on a pair of their own each, so that they cost the three junctions no link
        j = {"FR": 3, "RF": 4, "wrong": 5}.get(kind, r % 3)
        c1, c2, gap = 2 * j, 2 * j + 1, 4 + 30 * (j % 3)
        lead = int(J.rng.integers(5, 30))
        d1, d2 = {"FF": "FF", "RR": "RR", "FR": "FR", "RF": "RF", "wrong": "FN"}.get(kind, "FF")
        a, b = (c2, c1) if kind == "RR" else (c1, c2)
        if kind == "hit1_unmapped":
            a = -1
        elif kind == "hit2_unmapped":
            b = -1
        elif kind == "same_contig":
            b = a
        elif kind == "contig_is_n":
            a, b = (n_contigs, b) if r % 2 else (a, n_contigs)
        elif kind == "contig_minus_2":
            a, b = (-2, b) if r % 2 else (a, -2)
        read = rand_bytes(J.rng, lead + gap + 20 + r % 3)
        h = np.zeros(2, dtype=HIT_DTYPE)
        h[0] = (a, 1, lead, 7, 7 + lead - 1, r % 2, lead, ord(d1))
        h[1] = (b, lead + gap + 1, len(read), 1, len(read) - lead - gap, 0, len(read) - lead - gap, ord(d2))
        hits.append(h)
        reads.append(read)
        kinds.append(kind)
        if kind in ("FF", "RR", "FR", "RF", "wrong"):
            rows.append((r, len(read), lead, lead + gap + 1, a, b, ord(d1), ord(d2), (0, 0)))
    kept = np.array(rows, dtype=FR.REC_DTYPE)
    return HitJob("fill_hits", J.lens, reads, np.stack(hits), [0, 7], kinds, kept,
                  {"reads": len(plan), "kept": len(rows), "modes": [4, 4, 34, 34, 64]})   # (the FR and the RF pair are filled too)


@functools.lru_cache(maxsize=None)
def fill_scenarios():
    return [widths_x_spans(), column_ties(), host_path_late(), gapstat_runs(), gapstat_runs(last_single=True, name="gapstat_last_single"),
            more_units_than_waves()]


@functools.lru_cache(maxsize=None)
def fill_golden_scenarios():
    """the subset that goes to the real reference"""
    return [column_ties(), host_path_late(), widths_x_spans(GOLDEN_WIDTHS, GOLDEN_SPANS, "widths_x_spans_cut"),
            gapstat_runs(GOLDEN_RUN_LENGTHS, name="gapstat_runs_cut", one_long=1024)]


@functools.lru_cache(maxsize=None)
def fill_result(name):
    """FR.run on a scenario, computed once and shared"""
    f = {s.name: s for s in fill_scenarios() + fill_golden_scenarios() + [j.fill for j in slice_jobs()]}[name]
    return run_fill(f)


def run_fill(f):
    names = ["ctg_%d" % (2 * c + 1) for c in range(len(f.lens))]
    return FR.run(FR.Params(n=f.n), names, f.lens, [f.recs], ["x"], None, f.reads)


def filled_gaps(res):
    return [it for its in res["layout"] for it in its if it[0] == "gap" and it[1] > 0]


# ---- LINK -------------------------------------------------------------------------------------------------------------------

def naive_link_table(P, lens, recs):
    """add_data_into_link as the reference has it (link_func.cpp:430-473): record by record, per source node a list of
    [target, freq, size] in first-seen order, freq < 1023 guards both the count and the sum.  One record's class, nodes and gap
    come from scalar arithmetic of its own class (link_func.cpp:262-313, :367-415).  -> first, links, counters as LR.build_table"""
    n_nodes = 2 * len(lens) + 1
    chain = [[] for _ in range(n_nodes)]
    ctr = dict.fromkeys(LR.COUNTERS, 0)
    I = P.i

    def add(src, tgt, gap):
        for e in chain[src]:
            if e[0] == tgt:
                if e[1] < LR.FREQ_CAP:
                    e[1] += 1
                    e[2] += gap
                return
        chain[src].append([tgt, 1, gap])

    for c1, s1, e1, c2, s2, e2, d1, d2, _ in recs.tolist():
        cls = chr(d1) + chr(d2)
        if cls not in ("FR", "RF", "FF", "RR"):
            ctr["wrong"] += 1
            continue
        ctr[cls] += 1
        id1, id2, l1, l2 = 2 * c1 + 1, 2 * c2 + 1, int(lens[c1]), int(lens[c2])
        shape = cls if P.m == 0 else {"FR": "RF", "RF": "FR", "FF": "RR", "RR": "FF"}[cls]
        if shape == "FR":
            ctg1, ctg2, ctg3, ctg4, gap = id1, id1 + 1, id2, id2 + 1, I - (l1 - s1) - e2
        elif shape == "RF":
            ctg1, ctg2, ctg3, ctg4, gap = id2, id2 + 1, id1, id1 + 1, I - (l2 - s2) - e1
        elif shape == "FF":
            ctg1, ctg2, ctg3, ctg4, gap = id1, id1 + 1, id2 + 1, id2, I - (l1 - s1) - (l2 - s2)
        else:
            ctg1, ctg2, ctg3, ctg4, gap = id1 + 1, id1, id2, id2 + 1, I - (l1 - (l1 - e1)) - e2
        gap = int(FR.wrap32(gap))
        if gap > -LR.c_div(I, 2) and gap <= I:
            add(ctg1, ctg3, gap)
            add(ctg4, ctg2, gap)
    first = np.cumsum([0] + [len(c) for c in chain])
    flat = [e for c in chain for e in c]
    links = np.zeros(len(flat), dtype=LR.LINK_DTYPE)
    if flat:
        links["target"], links["freq"], links["size"] = zip(*flat)
    return first, links, ctr


class Lines(MLG.Scenario):
    """the golden maker's Scenario, its lines read back as records"""

    def recs(self):
        return LR.parse_2ctg("\n".join(self.lines), len(self.lens))


def gap_edges(I):
    return [-(I // 2), -(I // 2) + 1, I, I + 1]          # I > 0: -(I // 2) is C's -I / 2


def filter_edges(m, I):
    """for each of FR, RF, FF, RR four records on a contig pair of their own, with the gap at -(I/2), -(I/2) + 1, I, I + 1"""
    P = LR.Params(m=m, n=1, i=I)
    rng = np.random.default_rng(100 * m + I)
    lens = [int(x) for x in rng.integers(500, 3000, 8)]
    S = Lines(P, lens, rng)
    pairs = {}
    for j, cls in enumerate(("FR", "RF", "FF", "RR")):
        for g in gap_edges(I):
            S.record(cls, 2 * j, 2 * j + 1, g)
        pairs[cls] = (2 * j, 2 * j + 1)
    recs = S.recs()
    kept = gap_edges(I)[1:3]
    return Link("filter_edges_m%d_i%d" % (m, I), P, lens, recs, [0, 5, len(recs)],
                {"pairs": pairs, "freq": 2, "size": sum(kept), "lines": S.lines})


def cap_across_batches():
    """one key with 1022, 1023, 1024, 1025 and 2047 records (gap -7 for its first 1023 records in record order, +100 afterwards),
    each on a contig pair of its own, and one key whose first 1023 gaps are about 3 000 000 (-i 3000000; its sum exceeds 2^31),
    dealt round by round between records of other keys; the batches are cut behind round 1022, so the 1023rd and the 1024th
    record of every key lie in different batches"""
    P = LR.Params(m=0, n=1, i=BIG_INSERT)
    rng = np.random.default_rng(31)
    counts = CAP_COUNTS + (1030,)
    lens = []
    for _ in range(len(counts) + 4):
        lens += [int(rng.integers(400, 900)), BIG_INSERT + 500]   # long enough for  end2 = I - gap - (len1 - start1)
    S = Lines(P, lens, rng)
    key_of = []
    for r in range(max(counts)):
        for k, c in enumerate(counts):
            if r < c:
                if k < len(CAP_COUNTS):
                    g = -7 if r < LR.FREQ_CAP else 100
                else:
                    g = BIG_INSERT - 100 - r % 5 if r < LR.FREQ_CAP else 50
                S.record("FR", 2 * k, 2 * k + 1, g)
                key_of.append(k)
        o = len(counts) + r % 4                                # records of four other keys in between: none reaches the cap
        S.record("FR", 2 * o, 2 * o + 1, 30 + r % 40)
        key_of.append(o)
    recs = S.recs()
    key_of = np.array(key_of)
    cut = int(np.nonzero(key_of == 2)[0][LR.FREQ_CAP - 1]) + 1   # behind the 1023rd record of the key of 1024 records
    cut = int(np.nonzero(key_of[cut:] >= len(counts))[0][0]) + cut + 1   # ... and behind the rest of that round
    n = len(recs)
    big = sum(BIG_INSERT - 100 - r % 5 for r in range(LR.FREQ_CAP))
    sizes = {k: -7 * min(c, LR.FREQ_CAP) for k, c in enumerate(CAP_COUNTS)}
    return Link("cap_across_batches", P, lens, recs, [0, 1, cut // 2, cut, cut + 1, n],
                {"counts": counts, "key_of": key_of, "cut": cut, "sizes": sizes, "big_key": len(CAP_COUNTS), "big_size": big,
                 "lines": S.lines})


ORDER_TARGETS = 200


def first_seen_order():
    """node 1 (contig 0 forward) with 200 targets first seen in descending order over three batches; contig 1 forward with 40
    targets first seen in an order that is neither ascending nor descending; every target is seen a second time in ascending
    order, which must not move it.  The record's other entry (ctg4 -> ctg2) gives 200 reverse nodes one link each."""
    P = LR.Params(m=0, n=1, i=400)
    rng = np.random.default_rng(32)
    lens = [int(x) for x in rng.integers(500, 3000, 2 + ORDER_TARGETS)]
    S = Lines(P, lens, rng)
    targets = list(range(2, 2 + ORDER_TARGETS))
    second = [int(x) for x in np.random.default_rng(33).permutation(targets[:40])]
    assert second != sorted(second) and second != sorted(second, reverse=True)
    for k, t in enumerate(reversed(targets)):
        S.link(0, "+", t, "+", [10 + t % 50])
        if k < len(second):
            S.link(1, "+", second[k], "+", [60 + k])
    for t in targets:
        S.link(0, "+", t, "+", [20 + t % 50], alt=t % 2 == 0)
    for t in sorted(second):
        S.link(1, "+", t, "+", [5])
    recs = S.recs()
    n = len(recs)
    return Link("first_seen_order", P, lens, recs, [0, 70, 150, n],
                {"first": [2 * t + 1 for t in reversed(targets)], "second": [2 * t + 1 for t in second], "lines": S.lines})


LinkHitJob = namedtuple("LinkHitJob", "name P lens hits1 hits2 cuts kinds kept_rows expect")


def link_hits(m=0):
    """the LINK twin of fill_hits: first hits of the two mates for Scaffolder.add_hits, and the LR.PAIR_DTYPE rows a plain filter
    keeps (map_pair.cpp:315-323 and the range check)"""
    P = LR.Params(m=m, n=1, i=400)
    rng = np.random.default_rng(34)
    n_contigs = 10
    lens = [int(x) for x in rng.integers(500, 3000, n_contigs)]
    plan = [k for _ in range(4) for k in HIT_KINDS]
    plan = [plan[i] for i in np.random.default_rng(6).permutation(len(plan)).tolist()]
    S = Lines(P, lens, rng)
    h1, h2, rows = np.zeros(len(plan), dtype=HIT_DTYPE), np.zeros(len(plan), dtype=HIT_DTYPE), []
    for r, kind in enumerate(plan):
        j = r % 4
        cls = kind if kind in ("FF", "RR", "FR", "RF") else "FR"
        S.lines = []
        S.record(cls, 2 * j, 2 * j + 1, 20 + r)
        (c1, s1, e1, c2, s2, e2, d1, d2, _), = S.recs().tolist()
        if kind == "wrong":
            d2 = ord("N")
        elif kind == "hit1_unmapped":
            c1 = -1
        elif kind == "hit2_unmapped":
            c2 = -1
        elif kind == "same_contig":
            c2 = c1
        elif kind == "contig_is_n":
            c1, c2 = (n_contigs, c2) if r % 2 else (c1, n_contigs)
        elif kind == "contig_minus_2":
            c1, c2 = (-2, c2) if r % 2 else (c1, -2)
        h1[r] = (c1, 1, 100, s1, e1, 0, 100, d1)
        h2[r] = (c2, 1, 100, s2, e2, 1, 100, d2)
        if kind in ("FF", "RR", "FR", "RF", "wrong"):
            rows.append((c1, s1, e1, c2, s2, e2, d1, d2, (0, 0)))
    kept = np.array(rows, dtype=LR.PAIR_DTYPE)
    return LinkHitJob("link_hits_m%d" % m, P, lens, h1, h2, [0, 7, len(plan)], plan, kept, {"pairs": len(plan), "kept": len(rows)})


FILTER_JOBS = [(m, I) for m in (0, 1) for I in (400, 401, 1)]


@functools.lru_cache(maxsize=None)
def link_scenarios():
    return [filter_edges(m, I) for m, I in FILTER_JOBS] + [cap_across_batches(), first_seen_order()]
