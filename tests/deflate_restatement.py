"""The DEFLATE stage's rules (kernels in csrc/dbgk_gz.h) restated in plain Python: deflate(data, level, last) gives the
members byte for byte, members(data, level) lists them one by one with what the counters count.  CRC-32 is zlib's here: zlib is
the arbiter of the device's value, never its source."""
import struct
import zlib

import numpy as np

PIECE = 65280
HEAD = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0])
MARKER = HEAD + bytes([0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
COUNTERS = ("n_members", "out_bytes", "stored_members", "n_literals", "n_matches", "match_bytes")
MAX_LEVEL = 2
BLOCK = 256         # the matcher's chunk: a workgroup's width
HASH_BITS = 12
MAX_DIST, MAX_MATCH, MIN_MATCH = 32768, 258, 3
FAR = 4096           # a match of MIN_MATCH bytes farther back than this costs more than its literals: not used


def unlimited_depths(counts):
    """the lengths of a minimum-redundancy code for rising counts (Moffat and Katajainen, in place): ties go to the leaf"""
    a, n = list(counts), len(counts)
    if n == 1:
        return [1]
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or a[root] < a[leaf]:
            a[nxt] = a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] = a[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] += a[leaf]
            leaf += 1
    a[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    avbl, used, dpth, root, nxt = 1, 0, 0, n - 2, n - 1
    while avbl > 0:
        while root >= 0 and a[root] == dpth:
            used += 1
            root -= 1
        while avbl > used:
            a[nxt] = dpth
            nxt -= 1
            avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    return a


def code_lengths(freq, max_bits):
    """freq per symbol -> length per symbol.  The used symbols in rising (count, symbol) order; lengths above max_bits are cut to it,
    the code is made complete again by lengthening, one at a time, a code of the largest length below max_bits that has one; the
    lengths are dealt out from the most frequent symbol down"""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    lens = [0] * len(freq)
    if len(used) == 1:
        lens[used[0][1]] = 1
        return lens
    depths = unlimited_depths([f for f, _ in used])
    num = [0] * (max_bits + 2)
    for d in depths:
        num[min(d, max_bits)] += 1
    total = sum(num[l] << (max_bits - l) for l in range(1, max_bits + 1))
    while total > 1 << max_bits:
        num[max_bits] -= 1
        for l in range(max_bits - 1, 0, -1):
            if num[l]:
                num[l] -= 1
                num[l + 1] += 2
                break
        total -= 1
    j = len(used)
    for l in range(1, max_bits + 1):
        for _ in range(num[l]):
            j -= 1
            lens[used[j][1]] = l
    return lens


def canonical(lens):
    """RFC 1951, 3.2.2 -> the code of every symbol as it is written, first bit lowest"""
    top = max(lens)
    count = [0] * (top + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, c = [0] * (top + 2), 0
    for l in range(1, top + 1):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    out = []
    for l in lens:
        if not l:
            out.append(0)
            continue
        out.append(int(format(nxt[l], "0%db" % l)[::-1], 2))
        nxt[l] += 1
    return out


def run_lengths(seq):
    """-> [(symbol, extra)]: zeros as 18s of up to 138 while 11 and more are left, one 17 for 3..10, else single zeros; another
    length as itself, then 16s of up to 6 while 3 and more are left, then single lengths"""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                n = min(r, 138)
                out.append((18, n - 11))
                r -= n
            if r >= 3:
                out.append((17, r - 3))
                r = 0
        else:
            out.append((v, 0))
            r -= 1
            while r >= 3:
                n = min(r, 6)
                out.append((16, n - 3))
                r -= n
        out += [(v, 0)] * r
    return out


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):
        self.v |= v << self.n
        self.n += n


def len_symbol(n):
    """length 3..258 -> (symbol, extra bits, their value)"""
    l = n - 3
    if l < 8:
        return 257 + l, 0, 0
    if l == 255:
        return 285, 0, 0
    e = l.bit_length() - 3
    return 261 + 4 * e + ((l >> e) & 3), e, l & ((1 << e) - 1)


def dist_symbol(d):
    """distance 1..32768 -> (symbol, extra bits, their value)"""
    d -= 1
    if d < 4:
        return d, 0, 0
    n = d.bit_length() - 1
    e = n - 1
    return 2 * n + ((d >> e) & 1), e, d & ((1 << e) - 1)


def match_lengths(data, i, j, limit):
    """for arrays of positions j < i: how many bytes from j on equal those from i on, at most limit[.]"""
    n = np.zeros(i.size, dtype=np.int64)
    alive = np.ones(i.size, dtype=bool)
    for k in range(MAX_MATCH):
        alive &= k < limit
        idx = np.flatnonzero(alive)
        if not idx.size:
            break
        same = data[j[idx] + k] == data[i[idx] + k]
        alive[idx[~same]] = False
        n[idx[same]] += 1
    return n


def parse(piece):
    """the tokens of a piece at level 2: an int for a literal, (length, distance) for a match.  The piece is gone through in chunks of
    BLOCK positions.  Every position that has three bytes looks its hash up in a table that holds, per hash, the last position of the
    CHUNKS IN FRONT, then the chunk's positions enter the table (the largest wins).  Candidates: that position if it is at most
    MAX_DIST back, and the position one back.  Match lengths end at the piece's end and at MAX_MATCH; the distance-1 candidate wins if
    it is no shorter; under MIN_MATCH there is no match, nor with MIN_MATCH bytes farther back than FAR.  The parse is greedy from position 0."""
    data = np.frombuffer(piece, dtype=np.uint8).astype(np.int64)
    n = data.size
    pos = np.arange(n, dtype=np.int64)
    cand = np.full(n, -1, dtype=np.int64)
    if n >= MIN_MATCH:
        h = (((data[:-2] | data[1:-1] << 8 | data[2:] << 16) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - HASH_BITS)
        table = np.zeros(1 << HASH_BITS, dtype=np.int64)
        for c in range(0, n - 2, BLOCK):
            idx = pos[c:min(c + BLOCK, n - 2)]
            cand[idx] = table[h[idx]] - 1
            np.maximum.at(table, h[idx], idx + 1)
    limit = np.minimum(MAX_MATCH, n - pos)
    ok = (cand >= 0) & (pos - cand <= MAX_DIST) & (limit >= MIN_MATCH)
    la = np.zeros(n, dtype=np.int64)
    la[ok] = match_lengths(data, pos[ok], cand[ok], limit[ok])
    okb = (pos >= 1) & (limit >= MIN_MATCH)
    lb = np.zeros(n, dtype=np.int64)
    lb[okb] = match_lengths(data, pos[okb], pos[okb] - 1, limit[okb])
    la, lb, cand = la.tolist(), lb.tolist(), cand.tolist()
    tokens, i = [], 0
    while i < n:
        if lb[i] >= la[i] and lb[i] >= MIN_MATCH:
            tokens.append((lb[i], 1))
            i += lb[i]
        elif la[i] > MIN_MATCH or (la[i] == MIN_MATCH and i - cand[i] <= FAR):
            tokens.append((la[i], i - cand[i]))
            i += la[i]
        else:
            tokens.append(piece[i])
            i += 1
    return tokens


def dynamic_block(piece, level=1):
    """-> (the block's bytes, its parts).  Level 1: literals only, HLIT 257, one distance code of length 0.  Level 2: the tokens of
    parse(); HLIT and HDIST end at the last used symbol; no distance symbol: one code of length 0, one: length 1"""
    if level == 2:
        return dynamic_block_tokens(piece)
    freq = np.bincount(np.frombuffer(piece, dtype=np.uint8), minlength=257).tolist()
    freq[256] = 1
    lens = code_lengths(freq, 15)
    codes = canonical(lens)
    tokens = run_lengths(lens + [0])
    cl_freq = [0] * 19
    for s, _ in tokens:
        cl_freq[s] += 1
    cl_lens = code_lengths(cl_freq, 7)
    if sum(1 for f in cl_freq if f) == 1:   # a lone symbol gets a partner
        cl_lens[1 if cl_freq[0] else 0] = 1
    cl_codes = canonical(cl_lens)
    hclen = 19
    while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(0, 5)
    b.put(0, 5)
    b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl_lens[CL_ORDER[i]], 3)
    for s, extra in tokens:
        b.put(cl_codes[s], cl_lens[s])
        if s >= 16:
            b.put(extra, {16: 2, 17: 3, 18: 7}[s])
    head_bits = b.n
    # the literals: every code's bits, first bit first
    data = np.frombuffer(piece, dtype=np.uint8)
    L, Cd = np.array(lens[:256], dtype=np.int64)[data], np.array(codes[:256], dtype=np.int64)[data]
    k = np.arange(15, dtype=np.int64)
    bits = ((Cd[:, None] >> k) & 1).astype(np.uint8)[k[None, :] < L[:, None]]
    eob = [(codes[256] >> i) & 1 for i in range(lens[256])]
    head = [(b.v >> i) & 1 for i in range(head_bits)]
    allbits = np.concatenate([np.array(head, dtype=np.uint8), bits, np.array(eob, dtype=np.uint8)])
    return np.packbits(allbits, bitorder="little").tobytes(), {"freq": freq, "lens": lens, "cl_freq": cl_freq, "cl_lens": cl_lens, "tokens": tokens, "hclen": hclen,
                                                               "head_bits": head_bits, "bits": int(allbits.size)}


def block_header(lit_lens, dist_lens):
    """-> (Bits with the header of a dynamic block, parts)"""
    tokens = run_lengths(lit_lens + dist_lens)
    cl_freq = [0] * 19
    for s, _ in tokens:
        cl_freq[s] += 1
    cl_lens = code_lengths(cl_freq, 7)
    if sum(1 for f in cl_freq if f) == 1:
        cl_lens[1 if cl_freq[0] else 0] = 1
    cl_codes = canonical(cl_lens)
    hclen = 19
    while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(len(lit_lens) - 257, 5)
    b.put(len(dist_lens) - 1, 5)
    b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl_lens[CL_ORDER[i]], 3)
    for s, extra in tokens:
        b.put(cl_codes[s], cl_lens[s])
        if s >= 16:
            b.put(extra, {16: 2, 17: 3, 18: 7}[s])
    return b, {"cl_freq": cl_freq, "cl_lens": cl_lens, "tokens": tokens, "hclen": hclen, "head_bits": b.n}


def dynamic_block_tokens(piece):
    toks = parse(piece)
    freq, dfreq = [0] * 286, [0] * 30
    freq[256] = 1
    for t in toks:
        if isinstance(t, int):
            freq[t] += 1
        else:
            freq[len_symbol(t[0])[0]] += 1
            dfreq[dist_symbol(t[1])[0]] += 1
    lens = code_lengths(freq, 15)
    dlens = code_lengths(dfreq, 15) if any(dfreq) else [0] * 30
    codes, dcodes = canonical(lens), (canonical(dlens) if any(dlens) else [0] * 30)
    hlit = max([257] + [s + 1 for s in range(257, 286) if lens[s]])
    hdist = max([1] + [s + 1 for s in range(30) if dlens[s]])
    b, parts = block_header(lens[:hlit], dlens[:hdist])
    for t in toks:
        if isinstance(t, int):
            b.put(codes[t], lens[t])
        else:
            ls, le, lx = len_symbol(t[0])
            ds, de, dx = dist_symbol(t[1])
            b.put(codes[ls], lens[ls])
            b.put(lx, le)
            b.put(dcodes[ds], dlens[ds])
            b.put(dx, de)
    b.put(codes[256], lens[256])
    matches = [t for t in toks if not isinstance(t, int)]
    parts.update(freq=freq, lens=lens, dfreq=dfreq, dlens=dlens, hlit=hlit, hdist=hdist, bits=b.n, parse=toks, n_matches=len(matches),
                 match_bytes=sum(t[0] for t in matches), n_literals=len(toks) - len(matches))
    return b.v.to_bytes((b.n + 7) // 8, "little"), parts


def stored_block(piece):
    return b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece


def member(piece, level):
    """-> (the member's bytes, stored?, the dynamic block's parts or None)"""
    assert 0 < len(piece) <= PIECE and 0 <= level <= MAX_LEVEL
    block, parts = stored_block(piece), None
    if level >= 1:
        dyn, parts = dynamic_block(piece, level)
        if len(dyn) < len(block):
            block = dyn
        else:
            parts = dict(parts, rejected=True)
    size = 18 + len(block) + 8
    return HEAD + struct.pack("<H", size - 1) + block + struct.pack("<II", zlib.crc32(piece), len(piece)), (block[0] >> 1) & 3 == 0, parts


def members(data, level):
    data = bytes(data)
    return [member(data[i:i + PIECE], level) for i in range(0, len(data), PIECE)]


def deflate(data, level, last=True):
    """-> (bytes, info)"""
    ms = members(data, level)
    out = b"".join(m for m, _, _ in ms) + (MARKER if last else b"")
    dyn = [(i, p) for i, (_, stored, p) in enumerate(ms) if not stored]
    lit = sum(p["n_literals"] if level == 2 else min(PIECE, len(data) - i * PIECE) for i, p in dyn)
    return out, {"n_members": len(ms), "out_bytes": len(out), "stored_members": len(ms) - len(dyn), "n_literals": lit,
                 "n_matches": sum(p.get("n_matches", 0) for _, p in dyn), "match_bytes": sum(p.get("match_bytes", 0) for _, p in dyn)}


def walk(buf):
    """the members of a buffer by BSIZE -> [(offset, size, isize)]; raises ValueError for anything that is not this framing"""
    out, at = [], 0
    while at < len(buf):
        if len(buf) - at < 28:
            raise ValueError("cut short")
        if buf[at:at + 16] != HEAD:
            raise ValueError("not a member")
        size = struct.unpack_from("<H", buf, at + 16)[0] + 1
        if size < 28:
            raise ValueError("BSIZE too small")
        if len(buf) - at < size:
            raise ValueError("cut short")
        isize = struct.unpack_from("<I", buf, at + size - 4)[0]
        if isize > PIECE:
            raise ValueError("ISIZE above a piece")
        out.append((at, size, isize))
        at += size
    return out
