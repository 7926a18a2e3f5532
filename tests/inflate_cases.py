"""Crafted members of the INFLATE stage (csrc/dbgk_inflate_core.h, csrc/dbgk_inflate.h): the smallest shapes at which each path of the
decode can go wrong, built with the standard library alone -- zlib.compressobj for the streams zlib writes, a bit writer for the
ones it never would -- in the framing of tests/deflate_restatement.py.  valid_groups() -> {group: [(name, members, text)]}, where
`members` is one or more whole members and `text` what they inflate to; corrupt_cases() -> [(name, member, reason, device_only)],
each one mutation of a valid member that zlib refuses.  zlib is the arbiter: verdict(member) is what zlib.decompress(wbits=31) says."""
import struct
import zlib

import numpy as np

import deflate_cases as DC
import deflate_restatement as DR
import deflate_tokens as DT

PIECE = DR.PIECE
REASONS = ("OK", "BLOCK_TYPE", "STORED_LEN", "STORED_PAST", "TOO_MANY_SYMS", "CL_OVER", "CL_INCOMPLETE", "CODE_OVER", "CODE_INCOMPLETE",
           "REPEAT_FIRST", "REPEAT_PAST", "NO_EOB", "BAD_LENGTH", "BAD_DISTANCE", "DISTANCE_FAR", "TRUNCATED", "GARBAGE", "OUT_MORE", "OUT_LESS",
           "CRC", "FRAME")
R = {name: i for i, name in enumerate(REASONS)}


def frame(raw, text, crc=None, isize=None):
    """a deflate stream and the text it stands for -> the member"""
    size = 18 + len(raw) + 8
    assert size <= 65536 and len(text) <= PIECE, (size, len(text))
    return DR.HEAD + struct.pack("<H", size - 1) + raw + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize)


def verdict(member):
    """-> the bytes zlib inflates the member to, or None where it raises"""
    try:
        return zlib.decompress(member, wbits=31)
    except zlib.error:
        return None


def raw_deflate(text, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(text) + c.flush()


def zmember(text, *a, **k):
    return frame(raw_deflate(text, *a, **k), text)


def fasta_like(n, seed=3):
    rng = np.random.default_rng(seed)
    out, i = [], 0
    while sum(map(len, out)) < n:
        out.append(b">contig_%d length\n%s\n" % (i, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(rng.integers(50, 400))))))
        i += 1
    return b"".join(out)[:n]


# ---- a bit writer for the streams zlib never writes
class W:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):
        self.v |= v << self.n
        self.n += n
        return self

    def code(self, c, n):
        """a Huffman code: its first bit is its highest"""
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)
        return self

    def align(self):
        self.n += -self.n % 8
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def codes_of(lens):
    """canonical codes, first bit highest -> {symbol: (code, length)}"""
    top = max(lens) if lens else 0
    count = [0] * (top + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, c, out = [0] * (top + 2), 0, {}
    for l in range(1, top + 1):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


CL_LENS = [4] * 14 + [5] * 4 + [0]   # lengths 0..13 in four bits, 14, 15 and the repeats 16 and 17 in five: complete


def dynamic(w, lit_lens, dist_lens, tokens, final=1, seq=None, cl_lens=None, hlit=None, hdist=None, eob=True):
    """one dynamic block into w.  seq: the (symbol, extra) sequence of the lengths, by default every length as itself; tokens: an int
    for a literal, (length, distance) for a match, ("sym", s) for a bare literal/length symbol"""
    cl_lens = CL_LENS if cl_lens is None else cl_lens
    hclen = 19
    w.put(final, 1).put(2, 2).put((len(lit_lens) if hlit is None else hlit) - 257, 5).put((len(dist_lens) if hdist is None else hdist) - 1, 5).put(hclen - 4, 4)
    for s in DR.CL_ORDER:
        w.put(cl_lens[s], 3)
    cl = codes_of(cl_lens)
    for s, x in (seq if seq is not None else [(l, 0) for l in list(lit_lens) + list(dist_lens)]):
        w.code(*cl[s])
        if s >= 16:
            w.put(x, {16: 2, 17: 3, 18: 7}[s])
    body(w, codes_of(lit_lens), codes_of(dist_lens), tokens, eob)
    return w


def body(w, lit, dist, tokens, eob=True):
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "sym":
            w.code(*lit[t[1]])
        else:
            n, d = t
            s, e, x = DR.len_symbol(n)
            w.code(*lit[s]).put(x, e)
            s, e, x = DR.dist_symbol(d)
            w.code(*dist[s]).put(x, e)
    if eob:
        w.code(*lit[256])


def fixed(w, tokens, final=1, eob=True):
    w.put(final, 1).put(1, 2)
    body(w, codes_of(DT.FIXED_LIT), codes_of(DT.FIXED_DIST), tokens, eob)
    return w


def lens_for(used):
    """{symbol: length} -> the list of lengths up to the highest symbol"""
    out = [0] * (max(used) + 1)
    for s, l in used.items():
        out[s] = l
    return out


def stored_phases(raw):
    """the bit positions mod 8 at which the stream's stored blocks begin, by the token lister's own reads"""
    log, base = [], DT.Reader

    class Tracing(base):
        def bits(self, n):
            at = self.at
            v = base.bits(self, n)
            log.append((at, n, v))
            return v

    DT.Reader = Tracing
    try:
        DT.blocks(raw)
    finally:
        DT.Reader = base
    return [log[i][0] % 8 for i in range(len(log) - 2) if log[i][1] == 1 and log[i + 1][1:] == (2, 0) and log[i + 2][1] == 16]


def flush_cases():
    """Z_SYNC_FLUSH and Z_FULL_FLUSH at odd byte positions in mid-piece, until an empty stored block has begun at every bit phase"""
    text = DC.fastq_like(2400, seed=21)
    seen, out = set(), []
    for p in range(1, 1200, 2):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = c.compress(text[:p]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(text[p:2 * p + 301]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[2 * p + 301:]) + c.flush()
        ph = set(stored_phases(raw))
        if ph - seen:
            seen |= ph
            out.append(("flush_at_%d" % p, frame(raw, text), text))
        if len(seen) == 8:
            break
    assert seen == set(range(8)), seen
    return out


def far_match_member(dists=((258, 32768), (100, 32767))):
    """32 768 random bytes in a stored block, then a fixed block of matches at the largest distances there are: distance symbol 29
    with all 13 extra bits set, and one less -> (member, text)"""
    rnd = np.random.default_rng(41).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = W().put(0, 3).align().put(len(rnd) | (len(rnd) ^ 0xFFFF) << 16, 32).put(int.from_bytes(rnd, "little"), 8 * len(rnd))
    fixed(w, list(dists))
    out = bytearray(rnd)
    for n, d in dists:
        for _ in range(n):
            out.append(out[-d])
    return frame(w.bytes(), bytes(out)), bytes(out)


def valid_groups(own=True):
    g = {}
    # ---- the project's own members: every case of the deflater, at its three levels (the restatement takes seconds: own=False skips)
    if own:
        g["own"] = [("%s_level_%d" % (name, level), DR.deflate(data, level)[0], data) for name, data in DC.cases().items() for level in DC.LEVELS]
    # ---- zlib's
    rng = np.random.default_rng(31)
    rnd = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    texts = {"fastq": DC.fastq_like(PIECE, seed=13), "fasta": fasta_like(PIECE), "one_value": b"G" * PIECE, "period_2": b"AC" * (PIECE // 2),
             "period_3": b"ACG" * (PIECE // 3), "period_7": b"ACGTTGA" * (PIECE // 7), "distance_32768": rnd + rnd[:32512],
             "random": rng.integers(0, 256, 60000, dtype=np.uint8).tobytes()}
    z = []
    for name, text in texts.items():
        for level in (1, 6, 9):
            z.append(("%s_zlib_%d" % (name, level), zmember(text, level), text))
    z.append(("fixed_codes", zmember(DC.fastq_like(20000, seed=14) + bytes(range(144, 256)) * 3 + b"T" * 1000, 6, 8, zlib.Z_FIXED), None))
    z.append(("stored_one_block", zmember(texts["fastq"], 0), texts["fastq"]))
    z.append(("many_blocks", zmember(texts["fastq"], 6, 1), texts["fastq"]))
    z.append(("matches_at_32768_and_32767",) + far_match_member())
    g["zlib"] = [(n, m, verdict(m) if t is None else t) for n, m, t in z]
    # ---- small ones: flushes, hand-made blocks, the short pieces and the markers
    s = flush_cases()
    for level in (1, 6, 9):
        s.append(("fastq_600_zlib_%d" % level, zmember(DC.fastq_like(600, seed=15), level), DC.fastq_like(600, seed=15)))
    s.append(("fixed_small", zmember(b"ACGT" * 20 + bytes(range(140, 150)) + b"A" * 300, 6, 8, zlib.Z_FIXED), b"ACGT" * 20 + bytes(range(140, 150)) + b"A" * 300))
    s.append(("many_blocks_small", zmember(DC.fastq_like(2500, seed=16), 6, 1), DC.fastq_like(2500, seed=16)))
    s.append(("single_distance_symbol", frame(dynamic(W(), lens_for({65: 2, 256: 2, 257: 1}), [1], [65, (3, 1), (3, 1)]).bytes(), b"A" * 7), b"A" * 7))
    s.append(("no_distance_code", frame(dynamic(W(), lens_for({65: 1, 256: 1}), [0], [65, 65, 65]).bytes(), b"AAA"), b"AAA"))
    s.append(("empty_stored_blocks", frame(fixed(W(), [65], 0).put(0, 3).align().put(0xFFFF0000, 32).put(0, 3).align().put(0xFFFF0000, 32).put(1, 1).put(0, 2)
                                           .align().put(0xFFFE0001, 32).put(66, 8).bytes(), b"AB"), b"AB"))
    s.append(("empty_text", zmember(b""), b""))
    s.append(("marker_alone", DR.MARKER, b""))
    for n in (1, 2, 3):
        for level in (0, 6):
            s.append(("piece_of_%d_zlib_%d" % (n, level), zmember(b"ACG"[:n], level), b"ACG"[:n]))
    s.append(("markers_between_members", DR.MARKER + zmember(b"first\n") + DR.MARKER + DR.MARKER + zmember(b"second\n") + DR.MARKER, b"first\nsecond\n"))
    g["small"] = s
    return g


def corrupt_cases():
    """[(name, member, reason, device_only)]; device_only: the host walk refuses the member before any decode"""
    text = DC.fastq_like(900, seed=17)
    good = raw_deflate(text)
    ab = lens_for({65: 2, 66: 2, 256: 1})
    c = []
    c.append(("block_type_3", frame(b"\x07\x00", b""), R["BLOCK_TYPE"]))
    c.append(("stored_len_check", frame(b"\x01\x05\x00\xfa\xfe" + b"ACGTA", b"ACGTA"), R["STORED_LEN"]))
    c.append(("stored_runs_past_the_member", frame(b"\x01" + struct.pack("<HH", 1000, 1000 ^ 0xFFFF) + b"ACGTACGTAC", b"ACGTACGTAC"), R["STORED_PAST"]))
    for hlit, hdist in ((287, 1), (288, 1), (257, 31), (257, 32)):
        c.append(("hlit_%d_hdist_%d" % (hlit, hdist), frame(dynamic(W(), ab, [0], [65, 66], hlit=hlit, hdist=hdist).bytes() + bytes(8), b"AB"), R["TOO_MANY_SYMS"]))
    c.append(("cl_over_subscribed", frame(dynamic(W(), ab, [0], [65, 66], cl_lens=[1, 1, 1] + [0] * 16, seq=[]).bytes() + bytes(8), b"AB"), R["CL_OVER"]))
    c.append(("cl_incomplete", frame(dynamic(W(), ab, [0], [65, 66], cl_lens=[1] + [0] * 18, seq=[]).bytes() + bytes(8), b"AB"), R["CL_INCOMPLETE"]))
    c.append(("lit_over_subscribed", frame(dynamic(W(), lens_for({65: 1, 66: 1, 256: 1}), [0], []).bytes() + bytes(8), b"AB"), R["CODE_OVER"]))
    c.append(("lit_incomplete", frame(dynamic(W(), lens_for({65: 2, 256: 2}), [0], [65]).bytes(), b"A"), R["CODE_INCOMPLETE"]))
    c.append(("repeat_16_first", frame(dynamic(W(), ab, [0], [], seq=[(16, 0)] + [(0, 0)] * 255, eob=False).bytes() + bytes(8), b"AB"), R["REPEAT_FIRST"]))
    c.append(("repeat_past_the_lengths", frame(dynamic(W(), ab, [0], [], seq=[(l, 0) for l in ab] + [(17, 7)], eob=False).bytes() + bytes(8), b"AB"), R["REPEAT_PAST"]))
    c.append(("no_end_of_block_code", frame(dynamic(W(), lens_for({65: 1, 66: 1, 256: 0}), [0], [65, 66], eob=False).bytes() + bytes(8), b"AB"), R["NO_EOB"]))
    for s in (286, 287):
        c.append(("length_symbol_%d" % s, frame(fixed(W(), [65, ("sym", s)]).bytes() + bytes(4), b"AAAA"), R["BAD_LENGTH"]))
    for d in (30, 31):
        c.append(("distance_symbol_%d" % d, frame(fixed(W(), [65, ("sym", 257)], eob=False).code(d, 5).bytes() + bytes(4), b"AAAA"), R["BAD_DISTANCE"]))
    c.append(("distance_in_front_of_the_member", frame(fixed(W(), [65, (3, 2)]).bytes(), b"AAAA"), R["DISTANCE_FAR"]))
    c.append(("ends_in_mid_symbol", frame(good[:-2], text), R["TRUNCATED"]))
    c.append(("garbage_behind_the_final_block", frame(good + b"\x00\x55\xaa", text), R["GARBAGE"]))
    c.append(("more_output_than_isize", frame(good, text, isize=len(text) - 1), R["OUT_MORE"]))
    c.append(("less_output_than_isize", frame(good, text, isize=len(text) + 1), R["OUT_LESS"]))
    c.append(("wrong_crc", frame(good, text, crc=zlib.crc32(text) ^ 1), R["CRC"]))
    out = [(n, m, r, False) for n, m, r in c]
    m = bytearray(frame(good, text))
    m[0] = 0x1e
    out.append(("not_the_framing", bytes(m), R["FRAME"], True))
    return out


def split(members):
    """whole members back to back -> the list of them"""
    return [members[at:at + size] for at, size, _ in DR.walk(members)]


_LISTED = {}


def listed(member):
    """one member through the token lister, once per process -> (its counters, its largest distance)"""
    if member not in _LISTED:
        res, far = dict(n_stored=0, n_fixed=0, n_dynamic=0, n_literals=0, n_matches=0), 0
        for b in DT.gzip_member(member)[0]:
            res["n_" + b["type"]] += 1
            for t in b["tokens"]:
                if isinstance(t, int):
                    res["n_literals"] += 1
                else:
                    res["n_matches"] += 1
                    far = max(far, t[1])
        _LISTED[member] = (res, far)
    return _LISTED[member]


def counters(members):
    """what the token lister finds in whole members back to back -> {n_stored, n_fixed, n_dynamic, n_literals, n_matches}"""
    res = dict(n_stored=0, n_fixed=0, n_dynamic=0, n_literals=0, n_matches=0)
    for m in split(members):
        for f, v in listed(m)[0].items():
            res[f] += v
    return res
