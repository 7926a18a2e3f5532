"""Crafted batches for the ROWS stage (csrc/dbgk_maprow.h), small and aimed at the places where its kernels can go wrong: rows that end
at every interesting byte of a 16-byte vector, streams that end on and one behind the write kernel's tile, empty streams, every digit
count of every number, the identity's shapes, the classes of both modes.  A case is what capi.RowWriter.rows takes (and
tests/maprow_restatement.py restates): mode, delims, min_len, the contig table, and per side text / recs / bases / offsets / hits."""
import functools

import numpy as np

import maprow_restatement as RR

READS, PAIR = RR.READS, RR.PAIR
TILE = 4096
NO_HIT = (-1, -1, -1, -1, -1, 0, 0, ord("N"))
NAMES = [b"ctg1", b"scaffold_22", b"c", b"a_contig_with_a_rather_long_name|len=77|cov=12.5"]
LENGTHS = [1000, 50, 123456, 7]


def hit(contig, rs=1, re=30, cs=11, ce=40, mis=1, alen=30, direct="F"):
    return (contig, rs, re, cs, ce, mis, alen, ord(direct))


def make_side(headers, hits, reads=None, lens=None, final_newline=True):
    """the text is header line, read line, header line, ... (PAIR: header lines alone, the reads exist as lengths only)"""
    n = len(headers)
    assert len(hits) == n and (reads is None) != (lens is None)
    recs = np.zeros(n, dtype=RR.REC_DTYPE)
    text = bytearray()
    for i, h in enumerate(headers):
        recs[i]["head_pos"], recs[i]["head_len"] = len(text), len(h)
        text += h
        last = i == n - 1
        if not (last and not final_newline):
            text += b"\n"
        if reads is not None:
            if last and not final_newline:
                assert reads[i] == b""
            else:
                recs[i]["seq_pos"], recs[i]["seq_len"] = len(text), len(reads[i])
                text += reads[i] + b"\n"
    if reads is not None:
        lens = [len(q) for q in reads]
        bases = np.frombuffer(b"".join(reads), dtype=np.uint8)
    else:
        bases = None
    offsets = np.zeros(n + 1, dtype=np.uint64)
    if n:
        offsets[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64))
    H = np.zeros((n, 2), dtype=RR.HIT_DTYPE)
    for i, pair in enumerate(hits):
        for j, h in enumerate(pair):
            H[i, j] = h
    return {"text": bytes(text), "recs": recs, "bases": bases, "offsets": offsets, "hits": H}


def make(mode, delims, min_len, sides, names=NAMES, lengths=LENGTHS):
    return {"mode": mode, "delims": delims, "min_len": min_len, "names": list(names), "lengths": list(lengths), "sides": sides}


def read_of(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


# ---- READS ---------------------------------------------------------------------------------------------------------------------------

def reads_case(items, min_len=20, delims=b">@ \t\n", final_newline=True, names=NAMES, lengths=LENGTHS, seed=1):
    """items: (header, read or its length, hit a, hit b)"""
    rng = np.random.default_rng(seed)
    reads = [q if isinstance(q, bytes) else read_of(rng, q) for _, q, _, _ in items]
    side = make_side([h for h, _, _, _ in items], [(a, b) for _, _, a, b in items], reads=reads, final_newline=final_newline)
    return make(READS, delims, min_len, [side], names, lengths)


def reads_classes():
    A, B, C = hit(0), hit(1, 31, 60, 5, 34, 0, 30, "R"), hit(2, 2, 29, 100, 127, 2, 28)
    return [
        (b"@r1", 33, A, B),                          # 2ctg, one token
        (b"@r2 1:N:0:ACGT", 40, A, C),               # 2ctg, two tokens
        (b"@r3 x y z", 25, A, NO_HIT),               # 1ctg, four tokens: the first two count
        (b"@r4", 20, NO_HIT, NO_HIT),                # nothing mapped
        (b"@r5 e", 21, A, hit(0, 20, 21)),           # both on one contig: counted, not written
        (b"@r6 short", 19, A, B),                    # one base below min_len: neither written nor counted
        (b"@ \t ", 22, C, NO_HIT),                   # delimiters only: empty id
        (b"", 23, B, A),                             # an empty header line
        (b"@r9 desc\r", 24, A, B),                   # a '\r' is a token byte
        (b"\t@@r10>>x", 26, B, NO_HIT),              # leading delimiters, delimiters in a row
        (b"@r11", 27, NO_HIT, B),                    # b without a: nothing mapped
        (b"@r12 1", 20, C, B),
        (b"@r13 2", 50, C, NO_HIT),
    ]


# ---- PAIR ----------------------------------------------------------------------------------------------------------------------------

def pair_case(items, min_len=30, delims=b"@ \t", final_newline=True, names=NAMES, lengths=LENGTHS):
    """items: (header 1, length 1, hit 1, header 2, length 2, hit 2)"""
    s1 = make_side([x[0] for x in items], [(x[2], NO_HIT) for x in items], lens=[x[1] for x in items], final_newline=final_newline)
    s2 = make_side([x[3] for x in items], [(x[5], NO_HIT) for x in items], lens=[x[4] for x in items], final_newline=final_newline)
    return make(PAIR, delims, min_len, [s1, s2], names, lengths)


def pair_classes(mark=b"@"):
    A, B, C = hit(0), hit(1, 31, 60, 5, 34, 0, 30, "R"), hit(2, 2, 29, 100, 127, 2, 28)
    m = mark

    def P(k, l1, h1, l2, h2, extra=b""):
        return (m + b"p%d/1" % k + extra, l1, h1, m + b"p%d/2" % k + extra, l2, h2)
    return [
        P(1, 100, A, 100, B), P(2, 101, C, 99, A, b" 1:N:0"),     # 2ctg, two pairs in a row
        P(3, 100, A, 100, hit(0, 5, 34)), P(4, 30, B, 30, B),     # 1ctg
        P(5, 100, A, 100, NO_HIT), P(6, 100, C, 100, NO_HIT),     # gap, mate 1 only
        P(7, 100, NO_HIT, 100, B), P(8, 100, NO_HIT, 100, C),     # gap, mate 2 only
        P(9, 100, NO_HIT, 100, NO_HIT),                           # nothing mapped
        P(10, 100, A, 100, B),
        P(11, 29, A, 100, B),                                     # a short mate 1 between counted pairs
        P(12, 100, A, 100, C),
        P(13, 100, A, 29, B),                                     # a short mate 2
        P(14, 0, A, 0, B),                                        # both short
        P(15, 100, C, 100, NO_HIT),
        (m + b" \t", 64, A, b"", 65, B),                          # ids of no token
        (m + b"one", 64, A, m + b"two words more", 65, A),
    ]


# ---- numbers -------------------------------------------------------------------------------------------------------------------------

def digit_values():
    """a smallest and a largest value of every digit count 1 .. 10 that an int32 holds"""
    out = []
    for d in range(1, 11):
        out += [10 ** (d - 1), min(10 ** d - 1, 2 ** 31 - 1)]
    return out


def digits_pair():
    """every digit count in every numeric field: read lengths by the offsets (PAIR never touches the bases), contig lengths by the table,
    the four coordinates by the hits; all four row positions (first and second of a line, either mate alone)"""
    vals = digit_values()
    names = [b"n%d" % k for k in range(len(vals) + 1)]
    lengths = [min(v * 2 + 1, 2 ** 32 - 1) for v in vals] + [0]
    items = []
    for k, v in enumerate(vals):
        w = vals[len(vals) - 1 - k]
        h1, h2 = hit(k, v, w, w, v, k, 250), hit(len(vals), w, v, v, w, 0, 7, "R")
        items.append((b"@d%d" % k, v, h1, b"@e%d" % k, w, h2))
        items.append((b"@f%d" % k, w, h1, b"@g%d" % k, v, hit(k, 1, 2, 3, 4, 1, 9)))
        items.append((b"@h%d" % k, v, h1, b"@i%d" % k, v, NO_HIT))
        items.append((b"@j%d" % k, w, NO_HIT, b"@k%d" % k, v, h2))
    return pair_case(items, min_len=0, names=names, lengths=lengths)


def digits_reads():
    """READS prints the bases, so a read is as long as its number: one to seven digits here (a nine-digit read is 100 MB of bases);
    digits_pair reaches ten through the same kernel"""
    names = [b"n%d" % k for k in range(11)]
    lengths = [10 ** k - 1 for k in range(10)] + [2 ** 32 - 1]
    items = []
    for d in range(1, 8):
        L = 10 ** (d - 1) + d
        v = 10 ** (d + 2)
        items.append((b"@len%d x" % d, L, hit(d, L, v, v + 1, L, d, 100 + d), hit(10, v, L, 2 ** 31 - 1, v, 0, 5, "R")))
        items.append((b"@one%d" % d, L + 1, hit(d + 3, v, v, v, v, 3, 99), NO_HIT))
    return reads_case(items, min_len=0, names=names, lengths=lengths, seed=5)


IDENTITIES = [(0, 250), (250, 250), (1, 2), (1, 4), (1, 8), (1, 16), (1, 32), (1, 64), (3, 250), (7, 250), (1, 3), (2, 3), (9, 10), (1, 1 << 24),
              (1, 10 ** 7), (2, 10 ** 7), (999, 1000), (9999, 10000), (99999, 100000), (999995, 10 ** 6), (999999, 10 ** 6), (9999950, 10 ** 7),
              (9999990, 10 ** 7), (1234567, 7654321), (2 ** 31 - 2, 2 ** 31 - 1), (2 ** 30, 2 ** 31 - 1), (16777215, 16777216), (8388607, 8388608),
              (1, 2 ** 31 - 1), (0, 1), (1, 1), (123, 124), (124, 125)] + [(m, 250) for m in range(2, 40)] + [(a - 3, a) for a in range(100, 180, 7)] + \
             [(10 ** 6 - k, 10 ** 6) for k in range(2, 12)]
UNPRINTABLE = (20000002, 20000003)   # 1 - m / a rounds to 2^-24: 5.96046e-06 %


def identities():
    keep = [(m, a) for m, a in IDENTITIES if RR.percent(m, a) is not None]
    items = [(b"@i%d" % k, 30, hit(k % 3, 1, 30, 11, 40, m, a), NO_HIT) for k, (m, a) in enumerate(keep)]
    return reads_case(items)


def unprintable(mode):
    m, a = UNPRINTABLE
    assert RR.percent(m, a) is None
    if mode == READS:
        items = reads_classes()
        items.insert(5, (b"@u", 30, hit(0, 1, 30, 1, 30, m, a), NO_HIT))
        return reads_case(items)
    items = pair_classes()
    items.insert(7, (b"@u/1", 100, NO_HIT, b"@u/2", 100, hit(1, 1, 30, 1, 30, m, a)))
    return pair_case(items)


# ---- where rows and streams end ----------------------------------------------------------------------------------------------------------

def vector_ends():
    """1ctg rows (READS) whose ends fall 0, 1, 15 and 16 bytes into a 16-byte vector, each twice; the id's length places them"""
    targets = [0, 1, 15, 16, 1, 0, 16, 15, 8]
    items, at = [], 0
    for k, t in enumerate(targets):
        h = hit(k % 3, 1, 30, 11, 40, k, 30)
        bare = len(RR.row(b"", 30, dict(zip(RR.HIT_DTYPE.names, h)), NAMES, LENGTHS)) + 1
        pad = (t - (at + bare)) % 16
        if pad == 0:
            pad = 16
        items.append((b"@" + b"v" * pad, 30, h, NO_HIT))
        at += bare + pad
        assert at % 16 == t % 16
    return reads_case(items)


def stream_of(mode, stream, total, seed):
    """a case whose stream `stream` holds exactly `total` bytes: rows with ids of random lengths between items that land elsewhere, the
    last id padded to fit (READS prints it in both rows of a 2ctg line: there a one-digit coordinate mends the parity)"""
    A, B, B1 = hit(0, 1, 30, 11, 40, 1, 30), hit(3, 31, 60, 5, 34, 0, 30, "R"), hit(3, 31, 60, 5, 3, 0, 30, "R")

    def build(n_items, pad, tweak):
        rng = np.random.default_rng(seed)
        items = []
        for k in range(n_items):
            last = k == n_items - 1
            rid = b"@s%d" % k + (b"x" * pad if last else b"y" * int(rng.integers(0, 9)))
            second = B1 if last and tweak else B
            if mode == READS:
                items.append((rid + b" 2", 30, A, second if stream == 0 else NO_HIT))
                items.append((b"@other%d" % k, 30, A, NO_HIT if stream == 0 else B))
            else:
                items.append((rid, 100, A, b"@t%d/2" % k, 100, {0: second, 1: A, 2: NO_HIT}[stream]))
                items.append((b"@other%d" % k, 100, NO_HIT, b"@o", 100, NO_HIT))
        case = (reads_case if mode == READS else pair_case)(items)
        return case, len(RR.expected(case)["streams"][stream])
    n = 1
    while build(n + 1, 0, False)[1] <= total - 2:
        n += 1
    per = 2 if mode == READS and stream == 0 else 1
    tweak = (total - build(n, 0, False)[1]) % per != 0
    need = total - build(n, 0, tweak)[1]
    assert need >= 0 and need % per == 0
    case, size = build(n, need // per, tweak)
    assert size == total, (size, total)
    return case


def random_case(mode, n, seed):
    rng = np.random.default_rng(seed)
    names = [b"C%d" % (7 ** k) for k in range(12)]
    lengths = [int(rng.integers(1, 2 ** 32)) for _ in names]

    def rnd_hit():
        if rng.random() < 0.45:
            return NO_HIT
        a = int(rng.integers(1, 2000))
        return hit(int(rng.integers(0, len(names))), int(rng.integers(0, 10 ** int(rng.integers(1, 10)))), int(rng.integers(0, 5000)), int(rng.integers(0, 2 ** 31)),
                   int(rng.integers(0, 99999)), int(rng.integers(0, a + 1)), a, "FR"[int(rng.integers(0, 2))])

    def rnd_head(k):
        parts = [b"r%d" % k + b"z" * int(rng.integers(0, 20)), b"2:N:%d" % int(rng.integers(0, 1000)), b"more"][:int(rng.integers(1, 4))]
        return b"@" + b" ".join(parts)
    items = []
    for k in range(n):
        if mode == READS:
            items.append((rnd_head(k), int(rng.integers(15, 60)), rnd_hit(), rnd_hit()))
        else:
            items.append((rnd_head(k), int(rng.integers(25, 200)), rnd_hit(), rnd_head(k) + b"/2", int(rng.integers(25, 200)), rnd_hit()))
    return (reads_case if mode == READS else pair_case)(items, names=names, lengths=lengths)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["reads_classes"] = reads_case(reads_classes())
    c["pair_classes"] = pair_case(pair_classes())
    c["pair_classes_fasta"] = pair_case(pair_classes(b">"), delims=b"> \t")
    c["reads_n_0"] = reads_case([])
    c["pair_n_0"] = pair_case([])
    c["reads_only_1ctg"] = reads_case([x for x in reads_classes() if x[2][0] != -1 and x[3][0] == -1])          # streams 0 and 2 empty
    c["pair_only_gap"] = pair_case([x for x in pair_classes() if (x[2][0] == -1) != (x[5][0] == -1)])            # streams 0 and 1 empty
    c["reads_nothing_printed"] = reads_case([x for x in reads_classes() if x[2][0] == -1])
    A, B = hit(0), hit(1, 31, 60, 5, 34, 0, 30, "R")
    c["reads_header_ends_the_text_2ctg"] = reads_case([(b"@a 1", 5, A, B), (b"@last one", b"", A, B)], min_len=0, final_newline=False)
    c["reads_header_ends_the_text_1ctg"] = reads_case([(b"@a 1", 5, A, B), (b"@z", b"", B, NO_HIT)], min_len=0, final_newline=False)
    c["pair_header_ends_the_text"] = pair_case([(b"@a/1", 40, A, b"@a/2", 40, B), (b"@b/1 x", 40, A, b"@b/2 x", 40, NO_HIT)], final_newline=False)
    c["digits_pair"] = digits_pair()
    c["digits_reads"] = digits_reads()
    c["identities"] = identities()
    c["vector_ends"] = vector_ends()
    for total in (TILE, TILE + 1):
        c["reads_1ctg_of_%d_bytes" % total] = stream_of(READS, 1, total, 11)
        c["reads_2ctg_of_%d_bytes" % total] = stream_of(READS, 0, total, 12)
        c["pair_gap_of_%d_bytes" % total] = stream_of(PAIR, 2, total, 13)
    c["pair_2ctg_of_4096_bytes"] = stream_of(PAIR, 0, TILE, 14)
    c["pair_1ctg_of_8192_bytes"] = stream_of(PAIR, 1, 2 * TILE, 15)
    c["reads_random"] = random_case(READS, 700, 21)
    c["pair_random"] = random_case(PAIR, 700, 22)
    c["reads_unprintable"] = unprintable(READS)
    c["pair_unprintable"] = unprintable(PAIR)
    return c


# ---- the mapper's goldens as ROWS cases ---------------------------------------------------------------------------------------------------

def golden_rows_cases(golden_dir, case):
    """A case of tests/golden/map_cases or map_edge_cases -> [(name of the first reads file, ROWS case)], one per reads file (map_reads) or
    pair of files (map_pair): the records the reference's loop takes (tests/map_restatement.py), their restated hits, the contig table
    as the programs hold it.  The text of a side is rebuilt from the header lines; the reads of a pair exist as lengths."""
    import os

    import map_restatement as MR
    P = MR.params_of(case["args"])
    ids, contigs = MR.read_contig_file(os.path.join(golden_dir, case["contigs"]), P.l)
    X = MR.Index(contigs, P.k)
    names, lengths = [q.encode("latin-1") for q in ids], [len(q) for q in contigs]
    files = MR.read_lib_file(os.path.join(golden_dir, case["lib"]))
    out = []
    if case["program"] == "map_reads":
        for f in files:
            recs = MR.records_map_reads(os.path.join(golden_dir, f), P.fmt)
            reads = [r.encode("latin-1") for _, r in recs]
            side = make_side([h.encode("latin-1") for h, _ in recs], [tuple(MR.map_read(X, r, P, True)) for r in reads], reads=reads)
            out.append((os.path.basename(f), make(READS, b">@ \t\n", P.r, [side], names, lengths)))
    else:
        delims = b"@ \t" if P.fmt == 1 else b"> \t"
        for f1, f2 in zip(files[0::2], files[1::2]):
            recs = MR.records_map_pair(os.path.join(golden_dir, f1), os.path.join(golden_dir, f2), P.fmt)
            # (a line of file 1 that is no header maps the previous pair again: its entry repeats that pair's lines, the id included)
            heads, sides = [[], []], []
            for k, (h1, _, h2, _) in enumerate(recs):
                if h1[:1] == delims[:1].decode():
                    cur = (h1.encode("latin-1"), h2.encode("latin-1"))
                elif k == 0:
                    cur = (b"", b"")
                heads[0].append(cur[0])
                heads[1].append(cur[1])
            for m in (0, 1):
                reads = [r[1 + 2 * m].encode("latin-1") for r in recs]
                sides.append(make_side(heads[m], [(tuple(MR.map_read(X, r, P, False)[0]), NO_HIT) for r in reads], lens=[len(r) for r in reads]))
            out.append((os.path.basename(f1), make(PAIR, delims, P.r, sides, names, lengths)))
    return out
