"""The FORMAT stage's rule in plain Python (include/dbgk.h, FORMAT section): a join of byte strings.  record() is one record,
format_text() the records of a batch given as byte strings, format_batch() the same from the arrays the stage takes -- the text
with the records' header positions, the planes with their offsets, the suffixes.  tests/test_format_cpu.py anchors it to the host
writers and to files the reference wrote."""
import numpy as np

COUNTERS = ("n_records", "out_bytes", "head_bytes", "suffix_bytes", "seq_bytes")


def record(fmt, head, suffix, bases, quals, marker=0):
    if marker and len(head):
        head = bytes([marker]) + head[1:]
    if fmt == 1:
        return b"".join((head, suffix, b"\n", bases, b"\n+\n", quals, b"\n"))
    return b"".join((head, suffix, b"\n", bases, b"\n"))


def format_text(fmt, heads, reads, quals=None, suffixes=None, marker=0):
    """-> (text, info)"""
    assert fmt in (1, 2) and (fmt == 1) == (quals is not None)
    n = len(heads)
    suffixes = [b""] * n if suffixes is None else suffixes
    quals = [b""] * n if quals is None else quals
    assert len(reads) == len(quals) == len(suffixes) == n
    text = b"".join(record(fmt, h, s, r, q, marker) for h, s, r, q in zip(heads, suffixes, reads, quals))
    info = dict(n_records=n, out_bytes=len(text), head_bytes=sum(map(len, heads)), suffix_bytes=sum(map(len, suffixes)),
                seq_bytes=sum(map(len, reads)))
    return text, info


def pieces_of(text, recs, bases, quals, offsets):
    """the arrays the stage takes -> (heads, reads, quals or None) as byte strings"""
    text = bytes(text)
    off = [int(x) for x in offsets]
    b = np.asarray(bases, dtype=np.uint8).tobytes()
    heads = [text[int(r["head_pos"]):int(r["head_pos"]) + int(r["head_len"])] for r in recs]
    assert all(int(r["head_pos"]) + int(r["head_len"]) <= len(text) for r in recs)
    reads = [b[a:e] for a, e in zip(off[:-1], off[1:])]
    if quals is None:
        return heads, reads, None
    q = np.asarray(quals, dtype=np.uint8).tobytes()
    return heads, reads, [q[a:e] for a, e in zip(off[:-1], off[1:])]


def format_batch(fmt, text, recs, bases, quals, offsets, suffixes=None, marker=0):
    heads, reads, qs = pieces_of(text, recs, bases, quals, offsets)
    return format_text(fmt, heads, reads, qs, suffixes, marker)


def vectors(text):
    """the text as the stage leaves it on the device: whole 16-byte vectors, the pad 0"""
    out = np.zeros(-(-len(text) // 16) * 16, dtype=np.uint8)
    out[:len(text)] = np.frombuffer(text, dtype=np.uint8)
    return out
