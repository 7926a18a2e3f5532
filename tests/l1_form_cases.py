"""One case per level-1 kernel row of the product lists (dbg_assembly_amd/csrc/dbgk_l1_form.h: 110 instantiations): the handle,
the hooks, the entry point and the reads that make l1_plan select that row, and the launches such a batch makes.  Shared by
tests/test_l1_form_cpu.py (the plan of every case on the handle's real facts, through tests/l1_form_main.cpp) and
tests/l1_forms_gpu_steps.py (every case run on the GPU: Graph.l1_forms() and the result against the oracle).

Which handle reaches which rows (wide_d: how hash / size is computed -- 0: size < 2^31, 1: < 2^32, 2: 64-bit, 3: KFREQ direct blocks):
  graph, k = 31   the rows with k17 = 1 of the uniform and the prefix family, at the three table sizes; flat and flat-linear at wide_d 0, 1
  graph, k = 16   the rows with k17 = 0 of the uniform and the prefix family at wide_d 0 and 1; at wide_d 2 the two equal-length ones
  KFREQ, k = 13   direct blocks: the two wide_d = 3 rows; every other row with wide_d = 2 and k17 = 0 (ragged, linear, prefix), flat
                  and flat-linear at wide_d = 2
  WIDE, k = 63    wide-uniform and wide-flat at the three table sizes (2^32 slots and more: two passes, so two launches of the row)
Tables of 2^31 slots and more have 513 level-1 buckets: they take the linear forms unless l1_linear=0; the smallest table takes them
with l1_linear=1.

Lengths.  k = 31: W = 120 / 128 / 119 / 127 windows (L = 150 / 158 / 149 / 157), all Q = 8 lanes per read: 15 or 16 windows per lane,
reads that fill their lanes and reads that do not; 300 reads = two regular tiles of 128 reads and 44 reads for the general row.  The
plain equal-length rows take W = 105 / 112 (Q = 7, no regular tiles).  Other k: lengths with the same windows per lane; the ragged
rule (n_reads Q C <= 0.93 n_bases) decides which: tests/test_l1_form_cpu.py checks every recipe with the plan program.
"""
import collections
import random

N_READS = 300
MAX_READ_LEN = 250
EXPECTED_KMERS = 1000000       # dbgk_config.expected_kmers of the graph and WIDE handles: the record path
SLOTS = (1 << 26, 1 << 31, 1 << 32)   # table_slots of size class w = capi.find_next_prime_ref(SLOTS[w])
SIZE_CLASS = ("small", ">= 2^31", ">= 2^32")

Case = collections.namedtuple("Case", "row engine k max_read_len width hooks entry recipe passes launches")
# row       the form's text as l1_form_text() writes it (the key of cases())
# engine    "graph" (PARTITION), "kfreq" (KFREQ with direct blocks), "wide" (WIDE records)
# width     size class of the table: index into SLOTS / SIZE_CLASS (kfreq: 0, the table has 4^k bytes)
# hooks     DBGK_TEST_HOOKS of the batch
# entry     "push_reads", "push_reads_packed", "push_reads_packed_uniform"
# recipe    (name, L, c): reads(case) makes the read set
# passes    pushes of the whole read set (WIDE at 2^32 slots and more follows the pass protocol: 2)
# launches  the rows Graph.l1_forms() must report, in order

# Rows that no handle the library can create selects: {row: reason naming the conflicting conditions}.  None: in particular
# "prefix wide_d=2 k17=1" needs >= 2^32 slots and <= 960 level-1 buckets, and the planner gives a table just above 2^32 slots
# 513 buckets (r = 23: 1025 buckets of 2^22 slots would be more than the 1024 level 1 fans out to).
UNSELECTABLE = {}


def text(family, wide_d, c=0, ragged=0, lin=0, reg=0, packed=0, full=0, k17=0, has_dead=0, pipe=0):
    return "family=%s wide_d=%d c=%d ragged=%d lin=%d reg=%d packed=%d full=%d k17=%d has_dead=%d pipe=%d dbg=0" % (
        family, wide_d, c, ragged, lin, reg, packed, full, k17, has_dead, pipe)


def uniform(wide_d, c, ragged=0, lin=0, reg=0, packed=0, full=1, k17=0):
    return text("uniform", wide_d, c, ragged, lin, reg, packed, full, k17)


# read length by (k, windows per lane) of the recipes whose length the form constrains
EQUAL_LEN = {(31, 15): 135, (31, 16): 142,                 # plain equal lengths: W = 105 / 112, Q = 7
             (16, 15): 150, (16, 16): 143,                 # W = 135 (Q = 9) / 128
             (13, 15): 147, (13, 16): 140}                 # KFREQ: W = 135 / 128
RAGGED_LEN = {(31, 15): 150, (31, 16): 158,                # W = 120 / 128
              (16, 15): 120, (16, 16): 127,                # W = 105 / 112
              (13, 15): 102, (13, 16): 108}                # W = 90 / 96
LIN_LEN = {(31, 12): 150, (31, 8): 158,                    # W = 120 / 128 (the ragged rule holds for both)
           (16, 12): 135, (16, 8): 143, (13, 12): 132, (13, 8): 140}      # equal lengths: W = 120 / 128
LIN_RAGGED_LEN = {(31, 12): 150, (31, 8): 158, (16, 12): 111, (16, 8): 103, (13, 12): 108, (13, 8): 100}   # W = 96 / 88 at k = 16, 13
PREFIX_LEN = {(31, 15): 150, (31, 16): 158, (16, 15): 150, (16, 16): 143, (13, 15): 147, (13, 16): 140}
REG_LEN = {(15, 1): 150, (16, 1): 158, (15, 0): 149, (16, 0): 157}       # (c, full) at k = 31


def _hooks(width, lin, **more):
    """many level-1 buckets take the linear forms: forced on the small table, forced off on the big ones"""
    h = dict(more)
    if lin and width == 0:
        h["l1_linear"] = 1
    if not lin and width > 0:
        h["l1_linear"] = 0
    return h


def _graph_cases(out):
    def add(row, k, w, hooks, entry, recipe, launches=None):
        assert row not in out, row
        out[row] = Case(row, "graph", k, MAX_READ_LEN, w, hooks, entry, recipe, 1, launches or [row])

    for w in range(3):
        for c in (15, 16):
            # k = 31: the pipelined tile loop
            add(uniform(w, c, k17=1), 31, w, _hooks(w, 0), "push_reads_packed" if c == 15 else "push_reads", ("equal", EQUAL_LEN[31, c], c))
            add(uniform(w, c, ragged=1, k17=1), 31, w, _hooks(w, 0, l1_prefix=0), "push_reads" if c == 15 else "push_reads_packed",
                ("mixed", RAGGED_LEN[31, c], c))
            for packed in (0, 1):
                for full in (0, 1):
                    entry = "push_reads" if not packed else "push_reads_packed_uniform" if full else "push_reads_packed"
                    row = uniform(w, c, reg=1, packed=packed, full=full, k17=1)
                    add(row, 31, w, _hooks(w, 0), entry, ("equal", REG_LEN[c, full], c), [row, uniform(w, c, k17=1)])
            add(text("prefix", w, c, k17=1), 31, w, _hooks(w, 0, l1_prefix=1), "push_reads" if c == 15 else "push_reads_packed",
                ("mixed", PREFIX_LEN[31, c], c))
            # k = 16: the plain tile loop (at 2^32 slots the KFREQ handle runs all but the two equal-length rows)
            add(uniform(w, c), 16, w, _hooks(w, 0), "push_reads_packed_uniform" if c == 15 else "push_reads", ("equal", EQUAL_LEN[16, c], c))
            if w < 2:
                add(uniform(w, c, ragged=1), 16, w, _hooks(w, 0, l1_prefix=0), "push_reads" if c == 15 else "push_reads_packed",
                    ("mixed", RAGGED_LEN[16, c], c))
                add(text("prefix", w, c), 16, w, _hooks(w, 0, l1_prefix=1), "push_reads_packed" if c == 15 else "push_reads",
                    ("mixed", PREFIX_LEN[16, c], c))
        for c in (12, 8):
            add(uniform(w, c, lin=1, k17=1), 31, w, _hooks(w, 1), "push_reads_packed_uniform" if c == 12 else "push_reads", ("equal", LIN_LEN[31, c], c))
            add(uniform(w, c, ragged=1, lin=1, k17=1), 31, w, _hooks(w, 1), "push_reads" if c == 12 else "push_reads_packed",
                ("mixed", LIN_RAGGED_LEN[31, c], c))
            if w < 2:
                add(uniform(w, c, lin=1), 16, w, _hooks(w, 1), "push_reads" if c == 12 else "push_reads_packed_uniform", ("equal", LIN_LEN[16, c], c))
                add(uniform(w, c, ragged=1, lin=1), 16, w, _hooks(w, 1), "push_reads_packed" if c == 12 else "push_reads",
                    ("mixed", LIN_RAGGED_LEN[16, c], c))
        if w < 2:
            for dead in (0, 1):
                add(text("flat", w, has_dead=dead), 31, w, _hooks(w, 0, l1_prefix=0), "push_reads" if dead else "push_reads_packed", ("halves", 150, dead))
                add(text("flat-linear", w, lin=1, has_dead=dead), 31, w, _hooks(w, 1), "push_reads_packed" if dead else "push_reads", ("halves", 150, dead))


def _kfreq_cases(out):
    def add(row, hooks, entry, recipe):
        assert row not in out, row
        out[row] = Case(row, "kfreq", 13, MAX_READ_LEN, 0, hooks, entry, recipe, 1, [row])

    for c in (15, 16):
        add(uniform(3, c), {}, "push_reads_packed_uniform" if c == 15 else "push_reads", ("equal", EQUAL_LEN[13, c], c))
        add(uniform(2, c, ragged=1), dict(l1_prefix=0), "push_reads" if c == 15 else "push_reads_packed", ("mixed", RAGGED_LEN[13, c], c))
        add(text("prefix", 2, c), dict(l1_prefix=1), "push_reads_packed" if c == 15 else "push_reads", ("mixed", PREFIX_LEN[13, c], c))
    for c in (12, 8):
        add(uniform(2, c, lin=1), dict(l1_linear=1), "push_reads" if c == 12 else "push_reads_packed_uniform", ("equal", LIN_LEN[13, c], c))
        add(uniform(2, c, ragged=1, lin=1), dict(l1_linear=1), "push_reads_packed" if c == 12 else "push_reads", ("mixed", LIN_RAGGED_LEN[13, c], c))
    for dead in (0, 1):
        add(text("flat", 2, has_dead=dead), dict(l1_prefix=0), "push_reads" if dead else "push_reads_packed", ("halves", 150, dead))
        add(text("flat-linear", 2, lin=1, has_dead=dead), dict(l1_linear=1), "push_reads_packed" if dead else "push_reads", ("halves", 150, dead))


def _wide_cases(out):
    for w in range(3):
        passes = 2 if w == 2 else 1     # 1025 level-1 buckets of 2^22 slots: two passes over the input, each with its own level 1
        for row, hooks, entry, recipe in (
                (text("wide-uniform", w, pipe=1), {}, "push_reads", ("equal", 150, 8)),
                (text("wide-uniform", w, pipe=0), dict(wide_l1_plain=1), "push_reads_packed", ("equal", 150, 8)),
                (text("wide-flat", w, has_dead=0), {}, "push_reads_packed", ("mixed", 150, 8)),
                (text("wide-flat", w, has_dead=1), {}, "push_reads", ("trimmed", 150, 8))):
            assert row not in out, row
            out[row] = Case(row, "wide", 63, MAX_READ_LEN, w, hooks, entry, recipe, passes, [row] * passes)


def cases():
    """{row text: Case}, one per row of the product lists"""
    out = {}
    _graph_cases(out)
    _kfreq_cases(out)
    _wide_cases(out)
    return out


# ---- the reads ----------------------------------------------------------------------------------------------------------------------
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def mixed_lengths(L, k, c):
    """275 full-length reads and 25 cut to 60 .. L - 1 bases (tests/test_l1_form_cpu.py's MIXED at L = 150); one of the 25 has c m + 1
    windows: its last lane holds a single window"""
    cut = [60 + ((L - 1 - 60) * i) // 24 for i in range(25)]
    cut[12] = k + c * ((cut[12] - k) // c)
    assert min(cut) == 60 and max(cut) == L - 1 and (cut[12] - k + 1) % c == 1 and 60 < cut[12] < L
    return [L] * 275 + cut


def lengths(case):
    name, L, arg = case.recipe
    if name == "equal":
        return [L] * N_READS
    if name == "mixed":
        return mixed_lengths(L, case.k, arg)
    if name == "trimmed":                 # mixed lengths, three reads longer than max_read_len
        return mixed_lengths(L, case.k, arg)[:-3] + [case.max_read_len + 1, 300, 2 * case.max_read_len]
    if name == "halves":                  # half the reads at 70 bases; arg: three reads longer than max_read_len
        return [L] * 150 + [70] * (147 if arg else 150) + ([case.max_read_len + 1, 300, 2 * case.max_read_len] if arg else [])
    raise ValueError(name)


def reads(case):
    """the case's read set (a list of bytes), a function of the case alone.  Whatever the lengths: reads from both strands of a
    2000-base genome (coverage 20 and more: link counters above 1), one read 30 times, a poly-A and a poly-T read (key 0), a read with
    N, lower-case bases, and one byte outside ACGTNacgtn (read as A and counted: Stats.other_bytes)"""
    lens = lengths(case)
    rng = random.Random("%s %d %d %s" % (case.engine, case.k, case.width, case.recipe))
    genome = bytes(rng.choice(b"ACGT") for _ in range(2000))
    longest = max(lens)
    source = genome * (longest // len(genome) + 2)
    order = list(range(len(lens)))
    rng.shuffle(order)                    # (where in the batch the short, the long and the special reads lie)
    repeated = None
    out = [None] * len(lens)
    for n, i in enumerate(order):
        ln = lens[i]
        at = rng.randrange(len(genome))
        r = source[at:at + ln]
        if rng.random() < 0.5:
            r = r.translate(_COMP)[::-1]
        full = ln == lens[0]
        if full and n % (10 if lens.count(lens[0]) > 200 else 5) == 3:   # the repeated read: about 30 of the 300
            repeated = repeated or r
            r = repeated
        elif n == 0 or (full and n == 40):
            r = b"A" * ln
        elif n == 1 or (full and n == 41):
            r = b"T" * ln
        elif n == 2:
            r = r[:ln // 2] + b"N" + r[ln // 2 + 1:]
        elif n == 4:
            r = r[:ln - 7] + b"*" + r[ln - 6:]
        elif n == 5:
            r = r[:9] + r[9:40].lower() + r[40:]
        assert len(r) == ln
        out[i] = r
    return out
