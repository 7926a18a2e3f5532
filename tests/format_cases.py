"""Crafted batches for the FORMAT stage (tests/test_format_cpu.py, tests/format_gpu_steps.py): every case is the set of arrays the
stage takes -- the text that holds the headers, one record per header, the planes with their offsets, the suffixes -- built from
lists of byte strings by build().  What the stage makes of a case is tests/format_restatement.py's to say."""
import os

import numpy as np

import format_restatement as FR
from parse_restatement import REC_DTYPE

T = 4096   # DBGK_FMT_TILE
FASTQ, FASTA = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = os.path.join(ROOT, "tests", "golden", "clean_cases")
JUNK = 0xDEADBEEF   # in the fields of a record the stage does not use


def qual_of(i, n):
    return bytes(33 + (i * 7 + j * 3) % 41 for j in range(n))


def seq_of(i, n):
    return bytes(b"ACGTN"[(i + j * j + j // 3) % 5] for j in range(n))


def build(fmt, heads, reads, suffixes=None, marker=0, gaps=None, front=0, tail=b"\n", quals=None):
    """heads, reads (and for FASTQ the qualities, made by qual_of unless given) -> the case.  gaps[i]: the bytes of the text between
    header i - 1 and header i (default: a newline, nothing in front of the first); front: bytes of the planes in front of the first
    read, so offsets[0] == front; tail: the text behind the last header"""
    n = len(heads)
    assert len(reads) == n
    if gaps is None:
        gaps = [b""] + [b"\n"] * (n - 1)
    parts, recs, pos = [], np.full(n, JUNK, dtype=REC_DTYPE), 0
    for i, h in enumerate(heads):
        parts.append(gaps[i])
        pos += len(gaps[i])
        recs[i]["head_pos"], recs[i]["head_len"] = pos, len(h)
        parts.append(h)
        pos += len(h)
    text = b"".join(parts) + (tail if n else b"")
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[0] = front
    if n:
        offsets[1:] = front + np.cumsum([len(r) for r in reads], dtype=np.uint64)
    bases = np.frombuffer(b"#" * front + b"".join(reads), dtype=np.uint8)
    if fmt == FASTQ:
        quals = [qual_of(i, len(r)) for i, r in enumerate(reads)] if quals is None else quals
        assert [len(q) for q in quals] == [len(r) for r in reads]
        qplane = np.frombuffer(b"!" * front + b"".join(quals), dtype=np.uint8)
    else:
        qplane = None
    case = dict(fmt=fmt, marker=marker, text=text, recs=recs, bases=bases, quals=qplane, offsets=offsets, suffixes=suffixes)
    want, info = FR.format_text(fmt, heads, reads, quals if fmt == FASTQ else None, suffixes, marker)
    assert FR.format_batch(fmt, text, recs, bases, qplane, offsets, suffixes, marker) == (want, info)
    return case


def expected(case):
    """-> (text, info) of a case"""
    return FR.format_batch(case["fmt"], case["text"], case["recs"], case["bases"], case["quals"], case["offsets"], case["suffixes"], case["marker"])


def head_of(i, n, fmt=FASTQ):
    """a header of n bytes (n == 0: empty) that begins with the format's marker"""
    body = (b"r%d/" % i + b"abcdefghijklmnopqrstuvwxyz0123456789" * (n // 36 + 1))
    return ((b"@" if fmt == FASTQ else b">") + body)[:n]


def record_len(fmt, hl, sl, L):
    return hl + sl + 2 * L + 5 if fmt == FASTQ else hl + sl + L + 2


def sweep(fmt):
    """303 records whose header, suffix and read lengths each run through 0..100 three times in different orders, with gaps of
    0..20 bytes in the text: every source and destination position mod 16 and every pair of them mod 4, for every source"""
    heads, reads, sufs, gaps = [], [], [], []
    for rnd, (a, b, c) in enumerate(((1, 37, 73), (64, 10, 1), (23, 1, 50))):
        for i in range(101):
            k = rnd * 101 + i
            heads.append(head_of(k, (a * i + rnd) % 101, fmt))
            sufs.append((b" s%d:" % k + b"0123456789" * 10)[:(b * i + 2 * rnd) % 101])
            reads.append(seq_of(k, (c * i + 5 * rnd) % 101))
            gaps.append(b"\n" + b"x" * ((k * 5) % 21) if k else b"")
    return build(fmt, heads, reads, sufs, gaps=gaps, front=16 + 3)


def coverage(case):
    """for each source of a case -- header, suffix, bases and (FASTQ) quality -- the set of (source position, destination position)
    of the first byte of every piece that holds bytes"""
    fmt = case["fmt"]
    off = case["offsets"].astype(np.int64)
    sl = [len(s) for s in case["suffixes"]] if case["suffixes"] else [0] * len(case["recs"])
    out = {"head": set(), "suffix": set(), "bases": set()}
    if fmt == FASTQ:
        out["quals"] = set()
    dst, spos = 0, 0
    for i, r in enumerate(case["recs"]):
        hl, L = int(r["head_len"]), int(off[i + 1] - off[i])
        if hl:
            out["head"].add((int(r["head_pos"]), dst))
        if sl[i]:
            out["suffix"].add((spos, dst + hl))
        if L:
            out["bases"].add((int(off[i]), dst + hl + sl[i] + 1))
            if fmt == FASTQ:
                out["quals"].add((int(off[i]), dst + hl + sl[i] + 1 + L + 3))
        spos += sl[i]
        dst += record_len(fmt, hl, sl[i], L)
    return out


def covers_every_residue(case):
    for what, pairs in coverage(case).items():
        assert {s % 16 for s, _ in pairs} == set(range(16)) and {d % 16 for _, d in pairs} == set(range(16)), what
        assert {(s % 4, d % 4) for s, d in pairs} == {(a, b) for a in range(4) for b in range(4)}, what
    return True


def two_records(fmt, first_len, **kw):
    """a first record of first_len bytes of output (its read takes what its 7-byte header leaves) and a second one behind it"""
    hl = 7
    rest = first_len - record_len(fmt, hl, 0, 0)
    assert rest >= 0 and (fmt == FASTA or rest % 2 == 0), first_len
    L = rest // 2 if fmt == FASTQ else rest
    return build(fmt, [head_of(0, hl, fmt), head_of(1, 9, fmt)], [seq_of(0, L), seq_of(1, 40)], **kw)


def separator_at(border, shift):
    """FASTQ: one record in front, then a record whose "\\n+\\n" starts `shift` bytes in front of `border`, then one behind"""
    L = 21
    first = record_len(FASTQ, 5, 0, 10)
    hl = border - shift - first - 1 - L   # header, "\n", read -> the separator
    assert hl >= 1
    case = build(FASTQ, [head_of(0, 5), head_of(1, hl), head_of(2, 6)], [seq_of(0, 10), seq_of(1, L), seq_of(2, 30)])
    text, _ = expected(case)
    assert text[border - shift:border - shift + 3] == b"\n+\n" and text[border - shift - 1:border - shift] != b"\n"
    return case


def cases():
    """name -> case, in the order the GPU step runs them (a small batch follows the large ones on the same handle)"""
    out = {}
    for fmt, tag in ((FASTQ, "fastq"), (FASTA, "fasta")):
        out["empty_" + tag] = build(fmt, [], [])
        out["minimal_" + tag] = build(fmt, [head_of(0, 1, fmt)], [b""])
        out["no_bytes_at_all_" + tag] = build(fmt, [b"", b""], [b"", b""], tail=b"")
        out["sweep_0_100_" + tag] = sweep(fmt)
        for d in (-1, 0, 1, 2):   # its last byte is output byte T - 2 .. T + 1
            first = T + d
            if fmt == FASTQ and (first - record_len(fmt, 7, 0, 0)) % 2:
                # the read and its quality are equally long: an odd rest goes into a suffix of one byte
                hl, L = 7, (first - record_len(fmt, 7, 1, 0)) // 2
                out["first_record_ends_at_T%+d_%s" % (d, tag)] = build(fmt, [head_of(0, hl), head_of(1, 9)], [seq_of(0, L), seq_of(1, 40)],
                                                                          [b"~", b""])
            else:
                out["first_record_ends_at_T%+d_%s" % (d, tag)] = two_records(fmt, first)
            assert expected(out["first_record_ends_at_T%+d_%s" % (d, tag)])[0][:T + d].count(b"\n") == (4 if fmt == FASTQ else 2)
        big = 3 * T + 100
        out["pieces_of_3T_and_100_" + tag] = build(fmt, [head_of(0, 12, fmt), head_of(1, big, fmt), head_of(2, 3, fmt)],
                                                   [seq_of(0, 50), seq_of(1, big), seq_of(2, 20)], [b" a", b" S" * (big // 2), b""])
        n_empty = 3 * T
        out["run_of_3T_emptied_records_" + tag] = build(fmt, [head_of(i, 2 + i % 3, fmt) for i in range(n_empty + 2)],
                                                        [seq_of(0, 150)] + [b""] * n_empty + [seq_of(1, 151)])
        # a header at text byte 0 (every case has one) and one that ends at the text's last byte, n_text no multiple of 4
        for pad in (0, 1, 2):
            c = build(fmt, [head_of(0, 10, fmt), head_of(1, 11 + pad, fmt)], [seq_of(0, 33), seq_of(1, 35)], tail=b"")
            assert c["recs"][0]["head_pos"] == 0 and c["recs"][1]["head_pos"] + c["recs"][1]["head_len"] == len(c["text"])
            out["header_ends_the_text_%d_%s" % (len(c["text"]) % 4, tag)] = c
        raw = bytes([0x80, 0xFF, 0xC3, 0xA9])
        out["carriage_returns_and_high_bytes_" + tag] = build(
            fmt, [head_of(0, 8, fmt) + raw + b"\r", head_of(1, 1, fmt) + b"\r", b"\r"], [b"ACGTACGTAC\r", b"AC", raw], [b" x\r", raw, b""],
            quals=[bytes([0x80 + j for j in range(10)]) + b"\r", b"\xff\r", raw] if fmt == FASTQ else None)
        for marker in (ord(">"), ord("@")):
            out["marker_%02x_%s" % (marker, tag)] = build(fmt, [head_of(i, (0, 1, 2, 17, 40)[i % 5], FASTQ) for i in range(60)],
                                                          [seq_of(i, 10 + i) for i in range(60)],
                                                          [(b"", b" suffix", b"S")[i % 3] for i in range(60)], marker=marker)
        out["empty_headers_" + tag] = build(fmt, [b""] * 40, [seq_of(i, i) for i in range(40)], [b"", b"sfx"] * 20)
        for extra in (0, 1):
            heads, reads, total = [], [], 0
            while True:
                left = 16384 + extra - total
                L = 100
                if left < 2 * record_len(fmt, 8, 0, L):   # the last record takes what is left
                    rest = left - record_len(fmt, 8, 0, 0)
                    hl, L = (8 + rest % 2, rest // 2) if fmt == FASTQ else (8, rest)
                    heads.append(head_of(len(heads), hl, fmt))
                    reads.append(seq_of(len(reads), L))
                    break
                heads.append(head_of(len(heads), 8, fmt))
                reads.append(seq_of(len(reads), L))
                total += record_len(fmt, 8, 0, L)
            c = build(fmt, heads, reads)
            assert expected(c)[1]["out_bytes"] == 16384 + extra
            out["output_of_16384%+d_bytes_%s" % (extra, tag)] = c
    out["fasta_5000_records_of_3_bytes"] = build(FASTA, [b">"] * 5000, [b""] * 5000)
    assert expected(out["fasta_5000_records_of_3_bytes"])[1]["out_bytes"] == 15000
    assert expected(out["minimal_fastq"])[1]["out_bytes"] == 6 and expected(out["minimal_fasta"])[1]["out_bytes"] == 3
    for border, what in ((T, "tile"), (10 * 16, "vector")):
        for shift in (0, 1, 2, 3):
            out["separator_%d_bytes_in_front_of_a_%s_border" % (shift, what)] = separator_at(border, shift)
    out["small_after_large_fastq"] = build(FASTQ, [b"@last"], [b"ACGT"], [b" one"])
    return out
