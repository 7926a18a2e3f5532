"""A small inflate in plain Python that says what a deflate stream is made of: blocks(raw) lists, per block, its type, its code
lengths (dynamic blocks) and its tokens -- an int for a literal, (length, distance) for a match --, and returns the bytes.  For tests
that ask what the encoder chose; zlib remains the arbiter of validity."""
import struct

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
             24577]
DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32   # (symbols 30 and 31 take part in the code and never occur)


class Reader:
    def __init__(self, raw):
        self.v, self.n, self.at = int.from_bytes(raw, "little"), 8 * len(raw), 0

    def bits(self, n):
        if self.at + n > self.n:
            raise ValueError("stream cut short")
        r = (self.v >> self.at) & ((1 << n) - 1)
        self.at += n
        return r


def decoder(lens):
    """{(length, code as read bit by bit, first bit highest): symbol}; refuses an over-subscribed code, and an incomplete one unless
    it is the single code of length 1 or no code at all"""
    top = max(lens) if lens else 0
    count = [0] * (top + 2)
    for l in lens:
        if l:
            count[l] += 1
    left = 1
    for l in range(1, top + 1):
        left = (left << 1) - count[l]
        if left < 0:
            raise ValueError("over-subscribed code")
    used = sum(count)
    if left > 0 and not (used == 0 or (used == 1 and count[1] == 1)):
        raise ValueError("incomplete code")
    nxt, c, table = [0] * (top + 2), 0, {}
    for l in range(1, top + 1):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    for s, l in enumerate(lens):
        if l:
            table[l, nxt[l]] = s
            nxt[l] += 1
    return table


def symbol(r, table):
    c = 0
    for l in range(1, 16):
        c = c << 1 | r.bits(1)
        if (l, c) in table:
            return table[l, c]
    raise ValueError("no such code")


def blocks(raw):
    """-> ([{"type", "final", "tokens", and for dynamic blocks "lit_lens", "dist_lens", "cl_lens", "hclen", "cl_tokens"}], bytes, bits used)"""
    r, out, res = Reader(raw), bytearray(), []
    while True:
        final, kind = r.bits(1), r.bits(2)
        b = {"type": ("stored", "fixed", "dynamic")[kind] if kind < 3 else "reserved", "final": final, "tokens": []}
        if kind == 3:
            raise ValueError("reserved block type")
        if kind == 0:
            r.at += -r.at % 8
            n, nn = r.bits(16), r.bits(16)
            if n ^ nn != 0xFFFF:
                raise ValueError("stored length check")
            for _ in range(n):
                byte = r.bits(8)
                out.append(byte)
                b["tokens"].append(byte)
        else:
            if kind == 1:
                lit, dist = FIXED_LIT, FIXED_DIST
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = r.bits(3)
                t, lens, toks = decoder(cl), [], []
                while len(lens) < hlit + hdist:
                    s = symbol(r, t)
                    if s < 16:
                        lens.append(s)
                        toks.append((s, 0))
                    else:
                        n = r.bits({16: 2, 17: 3, 18: 7}[s])
                        toks.append((s, n))
                        if s == 16 and not lens:
                            raise ValueError("repeat with nothing in front")
                        lens += [lens[-1] if s == 16 else 0] * (n + {16: 3, 17: 3, 18: 11}[s])
                if len(lens) > hlit + hdist:
                    raise ValueError("a run passes the end of the lengths")
                lit, dist = lens[:hlit], lens[hlit:]
                if lit[256] == 0:
                    raise ValueError("no end-of-block code")
                b.update(lit_lens=lit, dist_lens=dist, cl_lens=cl, hclen=hclen, cl_tokens=toks)
            tl, td = decoder(lit), decoder(dist)
            while True:
                s = symbol(r, tl)
                if s < 256:
                    out.append(s)
                    b["tokens"].append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol above 285")
                    n = LEN_BASE[s - 257] + r.bits(LEN_EXTRA[s - 257])
                    d = symbol(r, td)
                    if d > 29:
                        raise ValueError("distance symbol above 29")
                    d = DIST_BASE[d] + r.bits(DIST_EXTRA[d])
                    if d > len(out):
                        raise ValueError("distance reaches in front of the output")
                    for _ in range(n):
                        out.append(out[-d])
                    b["tokens"].append((n, d))
        res.append(b)
        if final:
            return res, bytes(out), r.at


def gzip_member(buf):
    """one gzip member with BGZF's extra field (tests/deflate_restatement.py: HEAD) -> (blocks, bytes, crc, isize)"""
    size = struct.unpack_from("<H", buf, 16)[0] + 1
    res, out, used = blocks(buf[18:size - 8])
    if (used + 7) // 8 != size - 26:
        raise ValueError("the block does not end where the trailer starts")
    crc, isize = struct.unpack_from("<II", buf, size - 8)
    return res, out, crc, isize
