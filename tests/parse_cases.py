"""Crafted texts for the PARSE stage, shared by tests/test_parse_cpu.py (the restatement against the host readers) and
tests/parse_gpu_steps.py (the device against the restatement): the smallest shapes at which each kernel of csrc/dbgk_parse.h can go
wrong.  T is the text tile of the line kernels, E the output tile of the gather, CHUNK the lines one workgroup of the map scan takes."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = os.path.join(ROOT, "tests", "golden", "clean_cases")
T = 4096       # DBGK_PARSE_TEXT_TILE
E = 4096       # DBGK_CLEAN_COMPACT_TILE: kEmitTile
CHUNK = 2048   # parsek::kLineChunk; the spine scans 256 chunks a round
FASTQ, FASTA = 1, 2


def seq_of(rng, n):
    return np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, n)].tobytes()


def qual_of(i, n):
    """a function of (record, position): a swapped read or plane shows; never '\\n', sometimes '@'"""
    return ((33 + (i * 13 + np.arange(n) * 5) % 60).astype(np.uint8)).tobytes()


def fastq(rng, lens, first=0, head=lambda i: b"@r%d" % i):
    return b"".join(head(first + i) + b"\n" + seq_of(rng, n) + b"\n+\n" + qual_of(first + i, n) + b"\n" for i, n in enumerate(lens))


def fasta(rng, lens, first=0):
    return b"".join(b">r%d\n" % (first + i) + seq_of(rng, n) + b"\n" for i, n in enumerate(lens))


def with_total(rng, total):
    """read lengths 1..100 that sum to `total`"""
    lens = []
    while sum(lens) < total:
        lens.append(min(int(rng.integers(1, 101)), total - sum(lens)))
    return lens


def marker_lines(fmt, n_lines, junk):
    """n_lines lines that ALL begin with the marker, behind `junk` lines that do not: only the phase decides what is a header.  All
    lines have 6 bytes, so sequence and quality agree in length; what they hold depends on the line"""
    m = b"@" if fmt == FASTQ else b">"
    return b"".join(b"junk%d\n" % i for i in range(junk)) + b"".join(m + b"%05d\n" % (i * 7 % 100000) for i in range(n_lines))


def newline_at(rng, pos):
    """ordinary records, then one whose sequence line ends with its newline at byte `pos`, then ordinary records"""
    text = fastq(rng, [30, 41, 52])
    head = b"@edge\n"
    n = pos - len(text) - len(head)
    assert n > 0
    text += head + seq_of(rng, n) + b"\n+\n" + qual_of(3, n) + b"\n"
    assert text[pos:pos + 1] == b"\n" and text.count(b"\n", 0, pos) == 13
    return text + fastq(rng, [17, 5], first=4)


def cases():
    rng = np.random.default_rng(2024)
    c = {}
    # ---- degenerate
    c["empty"] = (FASTQ, b"")
    c["one_byte"] = (FASTQ, b"A")
    c["one_byte_marker"] = (FASTQ, b"@")
    c["one_byte_newline"] = (FASTQ, b"\n")
    c["no_newline"] = (FASTQ, b"@" + seq_of(rng, 99))
    c["no_newline_no_marker"] = (FASTQ, seq_of(rng, 100))
    c["header_only"] = (FASTQ, b"@h")
    c["header_only_newline"] = (FASTQ, b"@h\n")
    c["one_record"] = (FASTQ, b"@r\nACGTN\n+\nIIII@\n")
    c["one_record_no_final_newline"] = (FASTQ, b"@r\nACGTN\n+\nIIII@")
    c["norecords_fq"] = (FASTQ, open(os.path.join(CLEAN, "norecords.fq"), "rb").read())
    # ---- the rule
    c["quality_starts_with_at"] = (FASTQ, b"@r1\nACGT\n+\n@III\n@r2\nGGC\n+\n@@@\n@r3\nT\n+\nI\n")
    c["separator_starts_with_at"] = (FASTQ, b"@r1\nACGT\n@r1\n@III\n@r2\nGGC\n@\n@@@\n")
    c["junk_empty_lines_empty_header"] = (FASTQ, b"junk\n\n@r1\nACGT\n+\nIIII\nmore junk\n\n\n@\nGG\n+\nII\n+\n@r3\n\n+\n\n")
    c["crlf"] = (FASTQ, b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nGG\r\n+\r\nII\r\n")
    c["sequence_and_quality_differ"] = (FASTQ, b"@r1\nACGT\n+\nIII\n@r2\nGGC\n+\nIII\n@r3\nT\n+\nII\n@r4\n\n+\nI\n@r5\nAC\n+\n\n")
    c["truncated_in_sequence"] = (FASTQ, b"@r1\nACGT\n+\nIIII\n@r2\nGG")
    c["truncated_in_separator"] = (FASTQ, b"@r1\nACGT\n+\nIIII\n@r2\nGGC\n+")
    c["truncated_in_quality"] = (FASTQ, b"@r1\nACGT\n+\nIIII\n@r2\nGGC\n+\nII")
    c["fasta"] = (FASTA, b">r1\nACGT\n>r2\nTTGCA\n")
    c["fasta_no_final_newline"] = (FASTA, b">r1\nACGT\n>r2\nTTGCA")
    c["fasta_header_last"] = (FASTA, b">r1\nACGT\n>r2")
    c["fasta_junk_and_sequence_with_marker"] = (FASTA, b"junk\n\n>r1\n>ACGT\nmore junk\n@x\n>r2\n\n>r3\nGG\n")
    c["fasta_400_reads"] = (FASTA, fasta(rng, rng.integers(0, 120, 400)))
    # ---- state propagation: every line begins with the marker
    for n in (63, 64, 65, 255, 256, 257, 70001):
        for junk in (0, 1, 2, 3):
            c["all_marker_fastq_%d_lines_behind_%d" % (n, junk)] = (FASTQ, marker_lines(FASTQ, n, junk))
        for junk in (0, 1):
            c["all_marker_fasta_%d_lines_behind_%d" % (n, junk)] = (FASTA, marker_lines(FASTA, n, junk))
    # more than 256 chunks of lines: the spine carries its map from one round into the next
    n = 256 * CHUNK + 3 * CHUNK + 5
    c["all_marker_fastq_%d_short_lines_behind_1" % n] = (FASTQ, b"x\n" + b"@\n" * n)
    # ---- the line table
    for pos, tag in ((T - 1, "T_minus_1"), (T, "T"), (T + 1, "T_plus_1")):
        c["newline_at_" + tag] = (FASTQ, newline_at(rng, pos))
    c["line_of_3T_and_more"] = (FASTQ, fastq(rng, [50, 3 * T + 100, 60, 9]))
    c["lengths_0_100"] = (FASTQ, fastq(rng, [i % 101 for i in range(1200)], head=lambda i: b"@" + b"h" * (i * 7 % 23)))
    # ---- the gather's edges
    for total, tag in ((15, "15"), (16, "16"), (17, "17"), (E - 1, "E_minus_1"), (E, "E"), (E + 1, "E_plus_1")):
        c["total_" + tag] = (FASTQ, fastq(rng, [0] + with_total(rng, total) + [0]))
    c["all_emptied"] = (FASTQ, b"".join(b"@r%d\n" % i + seq_of(rng, 1 + i % 50) + b"\n+\nII" + b"I" * (i % 50) + b"\n" for i in range(300)))
    return c


TOTALS = {"15": 15, "16": 16, "17": 17, "E_minus_1": E - 1, "E": E, "E_plus_1": E + 1}
