"""Crafted inputs of the DEFLATE stage (csrc/dbgk_gz.h): the smallest shapes at which its kernels can go wrong.  cases() -> {name: bytes};
tests/test_deflate_cpu.py asserts that every case sits where its name claims, by the restatement."""
import random

import numpy as np

PIECE = 65280
LANE = 255          # kGzLaneBytes: the slice of a lane
BLOCK = 256         # kGzBlock
LEVELS = (0, 1, 2)
CHUNK = 256         # the matcher goes through a piece in chunks of a workgroup's width
FILL, BREAK = 0xFA, 0xFB
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
             24577]
CL_DEEP_SEED = 109  # found by search: see cl_deeper_than_7


def fastq_like(n, seed=5):
    """n bytes of four-line records of varying length"""
    rng = np.random.default_rng(seed)
    out, i = [], 0
    while sum(map(len, out)) < n:
        ln = int(rng.integers(30, 120))
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), ln))
        qual = bytes(rng.integers(35, 74, ln).astype(np.uint8))
        out.append(b"@read_%d/1\n%s\n+\n%s\n" % (i, seq, qual))
        i += 1
    return b"".join(out)[:n]


def with_counts(counts, seed=1):
    """a text in which byte value v occurs counts[v] times, in an order shuffled once"""
    buf = bytearray()
    for v, c in counts.items():
        buf += bytes([v]) * c
    random.Random(seed).shuffle(buf)
    return bytes(buf)


def fibonacci_counts():
    """22 byte values with counts 1, 1, 2, 3, 5, ..., sum 46 367.  The end-of-block symbol is a third 1, and with it every merge meets
    a tie that the construction gives to the leaf: its unrestricted code is only 12 deep."""
    c, a, b = {}, 1, 1
    for v in range(22):
        c[40 + 7 * v] = a
        a, b = b, a + b
    return c


def fibonacci_counts_with_eob():
    """21 byte values with counts 1, 2, 3, 5, ..., sum 46 366: the end-of-block symbol is the sequence's first 1, no merge meets a tie,
    and the unrestricted code is a chain 22 deep"""
    c = fibonacci_counts()
    del c[40]
    return c


def cl_deep_counts():
    """dyadic counts 2^(15 - l): the literal lengths are then exactly a tree's leaf depths, grown at random from CL_DEEP_SEED, and
    the symbols of the length sequence have counts whose unrestricted code is 8 deep"""
    rng = random.Random(CL_DEEP_SEED)
    leaves = [0]
    while len(leaves) < 20 + CL_DEEP_SEED % 200:
        i = rng.randrange(len(leaves))
        if leaves[i] >= 15:
            continue
        leaves[i] += 1
        leaves.append(leaves[i])
    syms = list(range(256))
    rng.shuffle(syms)
    leaves.remove(15)   # the end-of-block symbol's
    return {s: 1 << (15 - l) for s, l in zip(syms, leaves)}


def repeat_at(dist, length, seed, shift=0, cut=0):
    """a text in which `length` bytes at position p2 repeat the bytes `dist` in front, and nothing longer does: FILL bytes up to the
    first copy, the copy, FILL bytes, the second copy, a BREAK byte.  p2 is `shift` bytes in front of a chunk boundary of the matcher,
    and the first copy starts in an earlier chunk, as the matcher's table needs it (a hash of the same chunk is not in the table
    yet).  dist < length: the bytes have period dist.  cut: the text ends that many bytes into the second copy's end"""
    rng = random.Random(seed)
    p2 = CHUNK * max(1, -(-(dist + shift) // CHUNK)) - shift
    if dist >= length:
        x = bytes(rng.randrange(200) for _ in range(length))
        body = x + bytes([FILL]) * (dist - length) + x
    else:
        unit = bytes(rng.randrange(200) for _ in range(dist))
        body = (unit * (2 + length // dist))[:dist + length]
    text = bytes([FILL]) * (p2 - dist) + body + bytes([BREAK, BREAK + 1, BREAK + 2])
    return text[:len(text) - 3 - cut] if cut else text


def runs(lengths):
    """a run of n + 1 equal bytes for every n: a literal and a match of length n at distance 1 (two matches from 259 on)"""
    return b"".join(bytes([i % 256]) * (n + 1) for i, n in enumerate(lengths))   # (256 runs at the most: every byte value once)


def match_cases():
    c = {}
    for n in (3, 4, 257, 258):
        c["match_of_%d" % n] = repeat_at(1000, n, n)
    c["run_lengths_3_to_258"] = runs(range(3, 259))
    c["runs_of_259_and_261"] = runs([259, 261])
    for k, base in enumerate(DIST_BASE):
        top = (DIST_BASE[k + 1] if k < 29 else 32769) - 1
        for d in sorted({base, top}):
            if d > 1:   # (distance 1 is every run)
                c["distance_%d" % d] = repeat_at(d, 12, 7 * d + 1)
    c["distance_32769"] = repeat_at(32769, 12, 7)
    c["match_across_a_chunk_boundary"] = repeat_at(1000, 20, 5, shift=5)
    c["match_cut_by_the_end"] = repeat_at(512, 50, 6, cut=40)
    x = bytes(random.Random(8).randrange(200) for _ in range(40))
    c["repeat_across_the_member_boundary"] = fastq_like(PIECE - 40, seed=9) + x + x + fastq_like(500, seed=10)
    rng = np.random.default_rng(12)
    for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1):   # token counts around the lanes' slices
        c["sixteen_values_%d" % n] = rng.integers(0, 16, n, dtype=np.uint8).tobytes()
    return c


def cases():
    rng = np.random.default_rng(11)
    text = fastq_like(2 * PIECE + 1000)
    c = {"empty": b"", "one_byte": b"A", "two_bytes": b"AC", "three_bytes": b"ACG"}
    for n in range(601):
        c["fastq_len_%d" % n] = text[:n]
    for n in (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 2 * PIECE + 1):
        c["fastq_len_%d" % n] = text[:n]
    # around the multiples of a lane's slice: the last lane with bytes holds 1, 254, 255 of them
    for k in (3, 100, 200, BLOCK - 1):
        for d in (-1, 0, 1):
            c["slices_%d%+d" % (k, d)] = text[1000:1000 + k * LANE + d]
    c["one_value"] = b"A" * PIECE
    c["random_bytes"] = rng.integers(0, 256, PIECE + 1000, dtype=np.uint8).tobytes()        # two stored members
    c["random_then_text"] = rng.integers(0, 256, PIECE, dtype=np.uint8).tobytes() + text[:5000]   # a stored and a dynamic member
    c["fibonacci_counts"] = with_counts(fibonacci_counts())
    c["fibonacci_counts_with_eob"] = with_counts(fibonacci_counts_with_eob())
    c["cl_deeper_than_7"] = with_counts(cl_deep_counts())
    c["all_256_values"] = bytes(range(256)) * 40
    c["two_values"] = with_counts({10: 3000, 200: 1000})
    c["255_values_once"] = bytes(range(255))          # 256 codes of length 8: HCLEN at its smallest, and the block is not smaller
    # the second lane's first bit at every residue mod 64: k two-bit codes among the first lane's one-bit codes
    for k in range(64):
        c["second_lane_starts_%d_bits_later" % k] = b"b" * k + b"a" * (2 * LANE + 90 - k)
    c.update(match_cases())
    return c


def rounds_text():
    """more members than the member kernel's grid can hold on any device (8 workgroups per compute unit, 304 of them at the most), so
    that workgroups take a second piece: pieces rich in values first, then poor ones, a short one last.  No case is sized by a tile
    of the size scan: the stage has no scan kernel of its own, its sizes go through the library's scan (dbgk_internal_scan_lengths,
    rocPRIM's exclusive_scan), whose tile size is chosen inside that library and is not the stage's to pin.  The same call scans the
    far longer arrays of the EMIT, PAIR and PARSE stages in their tests."""
    a, b = fastq_like(240, seed=2), b"ACGT\n" * 48
    assert PIECE % len(a) == 0 and PIECE % len(b) == 0
    n_a, n_b = 8 * 304 + 1, 40
    return a * (PIECE // len(a) * n_a) + b * (PIECE // len(b) * n_b) + b"tail\n", n_a + n_b + 1
