"""CPU restatement of the cleaner's output stage (csrc/dbgk_emit.h, csrc/dbgk_clean_rule.h) in numpy: what a record makes of its
read as the two programs do it (host/clean_lowqual.cpp:85-117, host/clean_adapter.cpp:152-177), the compact offsets, the gather
of both planes with the N -> shift substitution, and the eight integer columns of the .stat file.  Pinned to the reference by
tests/test_clean_compact_cpu.py: applied to what tests/clean_restatement.py computes it gives lines 2 and 4 of every record and
the stat numbers of every golden the real reference wrote."""
import numpy as np

LOWQUAL, ADAPTER = 0, 1            # DBGK_CLEAN_KIND_*
HIT_DTYPE = np.dtype([("adapter", "<i4"), ("score", "<i4"), ("read_start", "<i4"), ("read_end", "<i4"), ("adapter_start", "<i4"),
                      ("adapter_end", "<i4")])                                              # dbgk_adapter_hit
BLOCK_DTYPE = np.dtype([("error_sum", "<f8"), ("start", "<i4"), ("length", "<i4"), ("trimmed", "<i4"), ("reserved", "<i4")])   # dbgk_lowqual_block
COUNTERS = ("reads", "raw_bases", "trimmed_reads", "trimmed_bases", "short_reads", "short_bases", "clean_reads", "clean_bases")


def hits_of(rows):
    """six-field tuples -> HIT_DTYPE"""
    rec = np.zeros(len(rows), dtype=HIT_DTYPE)
    for i, r in enumerate(rows):
        rec[i] = tuple(r)
    return rec


def blocks_of(rows):
    """(error_sum, start, length, trimmed) tuples -> BLOCK_DTYPE"""
    rec = np.zeros(len(rows), dtype=BLOCK_DTYPE)
    for i, r in enumerate(rows):
        rec[i] = tuple(r[:4]) + (0,)
    return rec


def cuts(kind, offsets, rec):
    """-> (start, length, trimmed) per read, 0-based, before the short-read filter.  A record that points outside its read (the
    kernels write none) keeps nothing"""
    L = np.diff(np.asarray(offsets, dtype=np.uint64)).astype(np.int64)
    if kind == LOWQUAL:
        trimmed = rec["trimmed"] != 0
        s, m = rec["start"].astype(np.int64) - 1, rec["length"].astype(np.int64)
        inside = (s >= 0) & (m >= 0) & (s + m <= L)
    else:
        trimmed = rec["adapter"] >= 0
        s, m = np.zeros(len(L), dtype=np.int64), rec["read_start"].astype(np.int64) - 1
        inside = (m >= 0) & (m <= L)
    start = np.where(trimmed & inside, s, 0)
    length = np.where(trimmed, np.where(inside, m, 0), L)
    return start, length, trimmed


def compact(kind, bases, quals, offsets, rec, shift=33, min_len=75):
    """-> (compact bases, compact qualities or None, compact offsets uint64[n + 1], counters).  After a lowqual batch the quality
    of every byte 'N' becomes `shift`; a result shorter than min_len becomes empty and keeps its place"""
    bases = np.asarray(bases, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    L = np.diff(offsets).astype(np.int64)
    start, m0, trimmed = cuts(kind, offsets, rec)
    short = m0 < min_len
    m = np.where(short, 0, m0)
    coff = np.zeros(n + 1, dtype=np.uint64)
    coff[1:] = np.cumsum(m)
    total = int(coff[n])
    owner = np.repeat(np.arange(n, dtype=np.int64), m)
    src = offsets[:-1].astype(np.int64)[owner] + start[owner] + (np.arange(total, dtype=np.int64) - coff[:-1].astype(np.int64)[owner])
    out_b = bases[src] if total else np.zeros(0, dtype=np.uint8)
    out_q = None
    if quals is not None:
        q = np.asarray(quals, dtype=np.uint8).copy()
        if kind == LOWQUAL:
            q[bases[:q.size] == ord("N")] = shift
        out_q = q[src] if total else np.zeros(0, dtype=np.uint8)
    clean = ~short if kind == ADAPTER else m > 0
    cnt = {"reads": n, "raw_bases": int(L.sum()), "trimmed_reads": int(trimmed.sum()), "trimmed_bases": int((L - m0)[trimmed].sum()),
           "short_reads": int(short.sum()), "short_bases": int(m0[short].sum()), "clean_reads": int(clean.sum()),
           "clean_bases": int(m[clean].sum())}
    return out_b, out_q, coff, cnt


def as_lines(plane, coff):
    b = np.asarray(plane, dtype=np.uint8).tobytes()
    return [b[int(coff[i]):int(coff[i + 1])] for i in range(len(coff) - 1)]


def lines_2_4(text):
    """the decompressed out.gz of either program -> (line 2 of every record, line 4 of every record), as bytes"""
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) % 4 == 1
    return [s.encode("latin-1") for s in lines[1:-1:4]], [s.encode("latin-1") for s in lines[3:-1:4]]


def stat_numbers(text):
    """the integer column of the eight lines of an out.stat of either program, named as dbgk_clean_compact_info names them"""
    vals = [int(line.split(":", 1)[1].split()[0]) for line in text.splitlines() if ":" in line]
    assert len(vals) == len(COUNTERS), text
    return dict(zip(COUNTERS, vals))


def trim_rule(kind, reads, quals, rows, shift=33, min_len=75):
    """the rule of capi.Cleaner.trim_adapter / trim_lowqual (and of the two programs) restated on byte strings, one read at a time:
    reads and quals as bytes, rows as hits_of / blocks_of take them -> (lines 2, lines 4, counters)"""
    seqs, quls = [], []
    cnt = dict.fromkeys(COUNTERS, 0)
    for s, q, row in zip(reads, quals, rows):
        n = len(s)
        cnt["reads"] += 1
        cnt["raw_bases"] += n
        if kind == ADAPTER:
            a, rs = row[0], row[2]
            if a >= 0:
                s, q = s[:rs - 1], q[:rs - 1]
                cnt["trimmed_reads"] += 1
                cnt["trimmed_bases"] += n - rs + 1
        else:
            start, length, trimmed = row[1:4]
            q = bytes(shift if c == ord("N") else v for c, v in zip(s, q))
            if trimmed:
                s, q = (s[start - 1:start - 1 + length], q[start - 1:start - 1 + length]) if start else (b"", b"")
                cnt["trimmed_reads"] += 1
                cnt["trimmed_bases"] += n - length
        short = len(s) < min_len
        if short:
            cnt["short_reads"] += 1
            cnt["short_bases"] += len(s)
            s, q = b"", b""
        if (not short) if kind == ADAPTER else len(s) > 0:
            cnt["clean_reads"] += 1
            cnt["clean_bases"] += len(s)
        seqs.append(s)
        quls.append(q)
    return seqs, quls, cnt


def pack(seqs):
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offsets


def fit(q, n):
    """a quality string laid under a read of n bytes: cut, or padded with zero bytes"""
    return (q + b"\0" * n)[:n]


def golden_batch(cases_dir, case):
    """a case of tests/golden/clean_cases as the batch the C ABI takes and what the reference's files say it becomes:
    -> dict(kind, reads, quals, opts, lines2, lines4, stat).  The two planes share one set of offsets, so a record whose strings
    differ in length (one, in mixed.fq) cannot be laid out as it is: for clean_lowqual the caller empties it, as the program does
    (raw_bases then lacks its bases, and `stat` is corrected by them); for clean_adapter its quality string is fitted under the read
    (`fit`), and so is the line 4 the reference wrote for it.  Every other record is compared as it stands."""
    import os
    import clean_restatement as CR
    o = CR.case_options(case)
    recs = CR.load_reads(os.path.join(cases_dir, case["input"]))
    want = CR.expected_outputs(cases_dir, case)
    lines2, lines4 = lines_2_4(want["out"])
    stat = stat_numbers(want["stat"])
    assert len(lines2) == len(recs) == stat["reads"]
    reads, quals = [], []
    for i, (_, s, q) in enumerate(recs):
        s, q = s.encode("latin-1"), q.encode("latin-1")
        if len(s) != len(q):
            if case["program"] == "clean_lowqual":
                stat["raw_bases"] -= len(s)
                s = q = b""
            else:
                q = fit(q, len(s))
                lines4[i] = fit(lines4[i], len(lines2[i]))
        reads.append(s)
        quals.append(q)
    return dict(kind=LOWQUAL if case["program"] == "clean_lowqual" else ADAPTER, reads=reads, quals=quals, opts=o, lines2=lines2,
                lines4=lines4, stat=stat)
