"""numpy restatement of the PAIR stage (include/dbgk.h, PAIR section): what merge_two_corr_files of the reference
(correct_error/correct.cpp:851-922) does to two files of records, as offsets, planes, source ids and counters.  No GPU, no library."""
import gzip
import os

import numpy as np

PAIRED, SINGLE = 0, 1
COUNTERS = ("pair_reads", "pair_bases", "single_reads", "single_bases")


def pack(seqs):
    """a list of bytes -> (uint8 plane, uint64 offsets)"""
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), offsets


def as_lines(plane, offsets):
    raw = np.asarray(plane, dtype=np.uint8).tobytes()
    return [raw[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def _gather(p1, p2, start, length, plane):
    """the reads (start, length) of plane 0 = p1 / 1 = p2 back to back -> (bytes padded with 0 to whole 16-byte vectors, offsets)"""
    off = np.zeros(len(length) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(length)
    total = int(off[-1])
    out = np.zeros((total + 15) // 16 * 16, dtype=np.uint8)
    if total:
        at = np.repeat(start.astype(np.int64) - off[:-1].astype(np.int64), length) + np.arange(total, dtype=np.int64)
        second = np.repeat(plane.astype(bool), length)
        a, b = np.asarray(p1, dtype=np.uint8), np.asarray(p2, dtype=np.uint8)
        if (~second).any():
            out[:total][~second] = a[at[~second]]
        if second.any():
            out[:total][second] = b[at[second]]
    return out, off


def split(b1, o1, b2, o2, q1=None, q2=None):
    """-> ({PAIRED: (bases, quals or None, offsets, ids), SINGLE: ...}, counters, max_len); the planes hold whole 16-byte vectors, the
    pad 0.  o1 / o2 need not start at 0: they index b1 / b2 as they are."""
    o1, o2 = np.asarray(o1, dtype=np.uint64), np.asarray(o2, dtype=np.uint64)
    assert len(o1) == len(o2) and (q1 is None) == (q2 is None)
    l1, l2 = np.diff(o1.astype(np.int64)), np.diff(o2.astype(np.int64))
    assert (l1 >= 0).all() and (l2 >= 0).all()
    both = (l1 > 0) & (l2 > 0)
    i = np.flatnonzero(both)
    length, start = np.empty(2 * len(i), dtype=np.int64), np.empty(2 * len(i), dtype=np.int64)
    length[0::2], length[1::2] = l1[i], l2[i]
    start[0::2], start[1::2] = o1[:-1].astype(np.int64)[i], o2[:-1].astype(np.int64)[i]
    rows = {PAIRED: (start, length, np.tile(np.array([0, 1]), len(i)), (2 * i[:, None] + np.array([0, 1])).reshape(-1))}
    # of a pair that is not kept at most one mate holds bytes: mate 1 if it is not empty, then mate 2 if it is not empty
    j = np.flatnonzero(~both & ((l1 > 0) | (l2 > 0)))
    second = l2[j] > 0
    rows[SINGLE] = (np.where(second, o2[:-1].astype(np.int64)[j], o1[:-1].astype(np.int64)[j]), np.where(second, l2[j], l1[j]),
                    second.astype(np.int64), 2 * j + second)
    out = {}
    for which, (start, length, plane, ids) in rows.items():
        bases, off = _gather(b1, b2, start, length, plane)
        quals = None if q1 is None else _gather(q1, q2, start, length, plane)[0]
        out[which] = (bases, quals, off, ids.astype(np.uint32))
    counters = {"pair_reads": 2 * len(i), "pair_bases": int(out[PAIRED][2][-1]), "single_reads": len(j), "single_bases": int(out[SINGLE][2][-1])}
    return out, counters, int(max(l1.max(initial=0), l2.max(initial=0)))


def stat_text(c):
    return "pair reads:   %d\npair bases:   %d\nsingle reads: %d\nsingle bases: %d\n" % tuple(c[f] for f in COUNTERS)


def merged_text(recs1, recs2):
    """two lists of (header line, sequence line) as bytes, one per record of <file>.correct.fa.gz -> (pair text, single text, stat text)
    through split(): the sequences go through the planes, the headers are attached by source id"""
    assert len(recs1) == len(recs2)
    b1, o1 = pack([s for _, s in recs1])
    b2, o2 = pack([s for _, s in recs2])
    out, counters, _ = split(b1, o1, b2, o2)
    heads = (recs1, recs2)
    text = []
    for which in (PAIRED, SINGLE):
        bases, _, off, ids = out[which]
        text.append(b"".join(heads[i & 1][i >> 1][0] + b"\n" + s + b"\n" for i, s in zip(ids.tolist(), as_lines(bases, off))))
    return text[0], text[1], stat_text(counters).encode()


def fa_records(path):
    """a two-lines-per-record file (gz or plain) -> [(header, sequence)]"""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        lines = f.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 2 == 0, path
    return list(zip(lines[0::2], lines[1::2]))


def rotate(recs):
    """mate file 2 of the goldens: the same records rotated by one"""
    return recs[1:] + recs[:1]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_cases")
CORRECT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "correct_k13")
# name of the case in pair_cases -> (its fq case in correct_k13, the options of the reference's run, both / only 1 / only 2 / neither)
CASES = {
    "default": ("default", [], (339, 34, 34, 5)),
    "c0": ("c0", ["-c", "0"], (94, 111, 111, 96)),
    "c3_m20_x5_r50": ("c3_m20_x5_r50", ["-c", "3", "-m", "20", "-x", "5", "-r", "50"], (405, 2, 2, 3)),
}


def classes(recs1, recs2):
    n = [0, 0, 0, 0]
    for (_, a), (_, b) in zip(recs1, recs2):
        n[0 if a and b else 1 if a else 2 if b else 3] += 1
    return tuple(n)
