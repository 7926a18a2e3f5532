"""The ROWS stage of include/dbgk.h restated in plain Python: what the host loops of bin/map_reads (host/map_reads.cpp, flush) and
bin/map_pair (host/map_pair.cpp, flush) write for one batch, from the same arrays the C entry takes -- per side the text with its
records, the n + 1 offsets (and for READS the bases), two hits per read -- and a contig table.  tests/test_maprow_cpu.py anchors it to
the files the real reference wrote."""
import numpy as np

READS, PAIR = 1, 2
HIT_DTYPE = np.dtype([("contig", "<i4"), ("read_start", "<i4"), ("read_end", "<i4"), ("contig_start", "<i4"), ("contig_end", "<i4"),
                      ("mismatches", "<i4"), ("align_len", "<i4"), ("direct", "<i4")])
REC_DTYPE = np.dtype([(f, "<u4") for f in ("head_pos", "head_len", "seq_pos", "seq_len", "qual_pos", "qual_len")])
IDENT_MAX = 11   # "0.000123456"


def split(line, delims):
    """split of map_func.cpp:33-53 on bytes: the maximal runs of bytes that are not in delims"""
    out, cur = [], bytearray()
    for c in line:
        if c in delims:
            if cur:
                out.append(bytes(cur))
                cur = bytearray()
        else:
            cur.append(c)
    if cur:
        out.append(bytes(cur))
    return out


def read_id(head, delims):
    """make_read_id of host/map_common.h"""
    t = split(head, delims)
    if not t:
        return b""
    return t[0] + b"-" + t[1] if len(t) > 1 else t[0]


def percent(mis, align_len):
    """`ostream << (float)(1.0 - (float)mis / align_len) * 100`, or None where the stream would not print plain digits"""
    with np.errstate(all="ignore"):
        q = np.float32(mis) / np.float32(align_len)
        identity = np.float32(1.0 - float(q))
        s = "%g" % float(np.float32(identity * np.float32(100)))
    return s.encode() if all(c in "0123456789." for c in s) else None


def row(rid, read_len, h, names, lengths):
    """Contigs::row; None when the identity is unprintable"""
    p = percent(int(h["mismatches"]), int(h["align_len"]))
    if p is None:
        return None
    c = int(h["contig"])
    return b"%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%s%%" % (rid, read_len, h["read_start"], h["read_end"], names[c], lengths[c], h["contig_start"],
                                                      h["contig_end"], bytes([int(h["direct"]) & 0xFF]), p)


def headers_of(side):
    t = bytes(side["text"])
    return [t[int(r["head_pos"]):int(r["head_pos"]) + int(r["head_len"])] for r in side["recs"]]


def expected(case):
    """-> {"streams": [bytes] * 3, "counters": [int] * 5, "unprintable": int}; with an unprintable row the streams are empty"""
    names, lengths, delims, min_len = case["names"], case["lengths"], case["delims"], case["min_len"]
    out = [[], [], []]
    cnt = [0] * 5
    bad = [0]

    def R(rid, L, h):
        r = row(rid, L, h, names, lengths)
        if r is None:
            bad[0] += 1
            return b""
        return r
    sides = case["sides"]
    ids = [[read_id(h, delims) for h in headers_of(s)] for s in sides]
    lens = [np.diff(np.asarray(s["offsets"], dtype=np.uint64).astype(np.int64)) for s in sides]
    n = len(lens[0])
    if case["mode"] == READS:
        s = sides[0]
        hits = np.asarray(s["hits"]).reshape(n, 2)
        bases = bytes(np.asarray(s["bases"], dtype=np.uint8)) if n else b""
        for i in range(n):
            L = int(lens[0][i])
            if L < min_len:
                continue
            cnt[0] += 1
            a, b = hits[i]
            if a["contig"] != -1:
                if b["contig"] != -1:
                    if a["contig"] != b["contig"]:
                        cnt[1] += 1
                        out[0].append(R(ids[0][i], L, a) + b"\t" + R(ids[0][i], L, b) + b"\n")
                        o = int(s["offsets"][i])
                        out[2].append(b">" + ids[0][i] + b"\n" + bases[o:o + L] + b"\n")
                    else:
                        cnt[4] += 1
                else:
                    cnt[2] += 1
                    out[1].append(R(ids[0][i], L, a) + b"\n")
            else:
                cnt[3] += 1
    else:
        h1 = np.asarray(sides[0]["hits"]).reshape(n, 2)[:, 0]
        h2 = np.asarray(sides[1]["hits"]).reshape(n, 2)[:, 0]
        for i in range(n):
            L1, L2 = int(lens[0][i]), int(lens[1][i])
            if L1 < min_len or L2 < min_len:
                continue
            cnt[0] += 1
            a, b = h1[i], h2[i]
            if a["contig"] != -1 and b["contig"] != -1:
                line = R(ids[0][i], L1, a) + b"\t" + R(ids[1][i], L2, b) + b"\n"
                if a["contig"] != b["contig"]:
                    cnt[1] += 1
                    out[0].append(line)
                else:
                    cnt[2] += 1
                    out[1].append(line)
            elif a["contig"] != -1 or b["contig"] != -1:
                cnt[3] += 1
                if a["contig"] != -1:
                    out[2].append(R(ids[0][i], L1, a) + b"\n")
                if b["contig"] != -1:
                    out[2].append(R(ids[1][i], L2, b) + b"\n")
            else:
                cnt[4] += 1
    streams = [b"".join(x) for x in out]
    if bad[0]:
        streams = [b"", b"", b""]
    return {"streams": streams, "counters": cnt, "unprintable": bad[0]}


HEAD1 = (b"#read_id\tread_length\talign_read_start\talign_read_end\tcontig_id\tcontig_length\talign_contig_start\talign_contig_end"
         b"\talign_direct\talign_identity%")
HEAD2 = HEAD1 + (b"\tread_id\tread_length\talign2_read_start\talign2_read_end\tcontig2_id\tcontig2_length\talign2_contig_start"
                 b"\talign2_contig_end\talign2_direct\talign2_identity%")
STAT_NAMES = {READS: ("total_read_num", "map_ctg_diff_num", "map_ctg_same_num", "map_no_no_num", "error_map_num"),
              PAIR: ("total_read_pair_num", "map_ctg_diff_num", "map_ctg_same_num", "map_ctg_gap_num", "map_no_no_num")}


def stat_text(mode, counters):
    """the .stat file of either program from the five counters (`double / uint64 * 100` through an ostream)"""
    total = counters[0]
    out = "\t%s: %d\n" % (STAT_NAMES[mode][0], total)
    for name, v in zip(STAT_NAMES[mode][1:], counters[1:]):
        out += "\t%s: %d  %s%%\n" % (name, v, ("%g" % (v / total * 100)) if total else "-nan")
    return out.encode()


def files_of(mode, streams, counters):
    """{file suffix: content} of one reads file (READS) or pair of files (PAIR): the header lines the programs write first, then the
    streams of all batches"""
    if mode == READS:
        return {".map_reads.2ctg.gz": HEAD2 + b"\n" + streams[0], ".map_reads.1ctg.gz": HEAD1 + b"\n" + streams[1],
                ".map_reads.2ctg.gz.reads.fa.gz": streams[2], ".map_reads.stat": stat_text(mode, counters)}
    return {".map_pair.2ctg.gz": HEAD2 + b"\n" + streams[0], ".map_pair.1ctg.gz": HEAD1 + b"\n" + streams[1],
            ".map_pair.gap.gz": HEAD1 + b"\n" + streams[2], ".map_pair.stat": stat_text(mode, counters)}
