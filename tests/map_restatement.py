"""Python restatement of the reference's map_reads and map_pair (link_scaffold/map_func.cpp, map_reads.cpp, map_pair.cpp):
get_align_seed, extend_align_region, the identity test in float arithmetic, the two driver loops with their file formats and
their output text.  The seed index comes from oracle_py.seed_index (pinned against the real chop_contig_to_kmerset).  Pinned
itself against goldens the real programs wrote (tests/golden/map_*, tests/test_map_cpu.py)."""
import gzip
import os
import re
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "k s l r i fmt")
Hit = namedtuple("Hit", "contig read_start read_end contig_start contig_end mismatches align_len direct")
NO_HIT = Hit(-1, -1, -1, -1, -1, 0, 0, ord("N"))

_CODE = [4] * 256  # alphabet[] of seqKmer.cpp:11-21; bytes from 128 on are an out-of-bounds read there and count as 4 here
for _ch, _v in (("A", 0), ("a", 0), ("N", 0), ("n", 0), ("C", 1), ("c", 1), ("G", 2), ("g", 2), ("T", 3), ("t", 3)):
    _CODE[ord(_ch)] = _v
_COMP = bytes(c if c in b"Nn" else b"TGCAN"[_CODE[c]] for c in range(256))  # one byte of rev_com_seq (seqKmer.cpp:83-91)
M64 = (1 << 64) - 1


def params_of(args):
    o = dict(zip(args[0::2], args[1::2]))
    return Params(k=int(o.get("-k", 31)), s=int(o.get("-s", 5)), l=int(o.get("-l", 125)), r=int(o.get("-r", 250)),
                  i=float(o.get("-i", 0.97)), fmt=int(o.get("-f", 1)))


def split(line, delim):
    return [t for t in re.split("[" + re.escape(delim) + "]+", line) if t]


def read_lib_file(path):
    """reading_lib_file (map_func.cpp:57-77)"""
    out = []
    for line in open(path).read().split("\n"):
        if line[:1] == "#":
            continue
        t = split(line, " \t\n")
        if t:
            out.append(t[0])
    return out


def read_contig_file(path, min_len):
    """read_contig_file (map_func.cpp:81-116) + the -l filter of main: a record without sequence in front of another header
    is dropped, the last record is always pushed, short contigs keep their index but become empty"""
    ids, seqs = [], []
    cur_id, cur = "", ""
    lines = open(path).read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for line in lines:
        if line[:1] == ">":
            if cur:
                ids.append(cur_id)
                seqs.append(cur)
            t = split(line, "> \t")
            cur_id = t[0] if t else ""
            cur = ""
        elif line:
            cur += line
    ids.append(cur_id)
    seqs.append(cur)
    return ids, [q if len(q) >= min_len else "" for q in seqs]


def open_text(path):
    """igzstream: gzip or plain"""
    with open(path, "rb") as f:
        magic = f.read(2)
    data = gzip.open(path, "rb").read() if magic == b"\x1f\x8b" else open(path, "rb").read()
    lines = data.decode("latin-1").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return lines


class Index:
    def __init__(self, contigs, k):
        from oracle import oracle_py as orc
        nodes = orc.seed_index(contigs, k)
        self.k = k
        self.nodes = {int(n["kmer"]): (int(n["id"]), int(n["pos"]), int(n["freq"]), int(n["direct"])) for n in nodes}
        self.contigs = [q.encode("latin-1") if isinstance(q, str) else bytes(q) for q in contigs]


def window_key(read, i, k):
    """seq2bit (codes OR-ed in unmasked), get_rev_com_kbit, the canonical pick (map_func.cpp:188-199)"""
    kbit = 0
    for c in read[i:i + k]:
        kbit = ((kbit << 2) | _CODE[c]) & M64
    inv = ~kbit & M64
    rc = 0
    for j in range(32):  # reverse the 32 two-bit groups
        rc |= ((inv >> (2 * j)) & 3) << (2 * (31 - j))
    rc >>= 64 - 2 * k
    return (kbit, 1) if kbit < rc else (rc, 0)


def get_align_seed(X, read, search_start, P):
    """map_func.cpp:181-237 with search_end = the read's length -> (contig, cs, ce, rs, re, direct) or None"""
    k, s = X.k, P.s
    for i in range(search_start - 1, len(read) - k - s + 1):
        kmer, direct = window_key(read, i, k)
        n1 = X.nodes.get(kmer)
        if n1 is None or n1[2] != 1:
            continue
        kmer2, _ = window_key(read, i + s, k)
        n2 = X.nodes.get(kmer2)
        if n2 is None or n2[2] != 1 or n2[0] != n1[0] or abs(n2[1] - n1[1]) != s:
            continue
        if direct == n1[3]:
            return n1[0], n1[1] + 1, n2[1] + k, i + 1, i + s + k, "F"
        return n1[0], n2[1] + 1, n1[1] + k, i + 1, i + s + k, "R"
    return None


def extend_align_region(read, contig, cs, ce, rs, re_, direct):
    """map_func.cpp:241-299 -> (cs, ce, rs, re, mis_match, align_len)"""
    L = len(read)
    align_len = re_ - rs + 1
    mis = 0
    if direct == "R":
        read = read[::-1].translate(_COMP)
        rs, re_ = L - re_ + 1, L - rs + 1
    while rs > 1:
        if cs - 1 < 1:
            break
        rs -= 1
        cs -= 1
        align_len += 1
        if read[rs - 1] != contig[cs - 1]:
            mis += 1
    while re_ < L:
        if ce - 1 >= len(contig) - 1:
            break
        re_ += 1
        ce += 1
        align_len += 1
        if read[re_ - 1] != contig[ce - 1]:
            mis += 1
    if direct == "R":
        rs, re_ = L - re_ + 1, L - rs + 1
    return cs, ce, rs, re_, mis, align_len


def identity(mis, align_len):
    """float identity = 1.0 - (float)mis_match / align_len"""
    q = np.float32(mis) / np.float32(align_len)
    return np.float32(1.0 - float(q))


def accepted(mis, align_len, min_identity):
    return not (float(identity(mis, align_len)) < min_identity)


def percent(mis, align_len):
    """`identity * 100` through an ostream at its default precision"""
    return "%g" % float(np.float32(identity(mis, align_len) * np.float32(100)))


def map_one(X, read, search_start, P):
    seed = get_align_seed(X, read, search_start, P)
    if seed is None:
        return NO_HIT
    ctg, cs, ce, rs, re_, direct = seed
    cs, ce, rs, re_, mis, alen = extend_align_region(read, X.contigs[ctg], cs, ce, rs, re_, direct)
    return Hit(ctg if accepted(mis, alen, P.i) else -1, rs, re_, cs, ce, mis, alen, ord(direct))


def map_read(X, read, P, second):
    """the two hits of one read as dbgk_map_reads returns them (map_reads.cpp:456-498, map_pair.cpp:284-311)"""
    h1 = h2 = NO_HIT
    if len(read) < P.r or len(read) < X.k + P.s:
        return h1, h2
    h1 = map_one(X, read, 1, P)
    if second and h1.contig != -1 and h1.read_end < len(read) and len(read) - h1.read_end >= X.k + P.s:
        h2 = map_one(X, read, h1.read_end + 1, P)
    return h1, h2


def read_id(head, delim):
    t = split(head, delim)
    return t[0] + ("-" + t[1] if len(t) > 1 else "")


def records_map_reads(path, fmt):
    """map_reads.cpp:295-320 -> [(header line, read)]"""
    lines = open_text(path)
    out, i = [], 0
    mark, step = ("@", 4) if fmt == 1 else (">", 2)
    while i < len(lines):
        if lines[i][:1] == mark:
            out.append((lines[i], lines[i + 1] if i + 1 < len(lines) else ""))
            i += step
        else:
            i += 1
    return out


def row(rid, read, h, ids, contigs):
    return "%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%s%%" % (rid, len(read), h.read_start, h.read_end, ids[h.contig], len(contigs[h.contig]),
                                                        h.contig_start, h.contig_end, chr(h.direct), percent(h.mismatches, h.align_len))


HEAD1 = ("#read_id\tread_length\talign_read_start\talign_read_end\tcontig_id\tcontig_length\talign_contig_start\talign_contig_end"
         "\talign_direct\talign_identity%")
HEAD2 = HEAD1 + ("\tread_id\tread_length\talign2_read_start\talign2_read_end\tcontig2_id\tcontig2_length\talign2_contig_start"
                 "\talign2_contig_end\talign2_direct\talign2_identity%")


def ratio(n, total):
    return "%g" % (n / total * 100) if total else "-nan"


def run_map_reads(X, ids, reads_file, P, hits=None):
    """one reads file -> {suffix: text}; `hits` (n, 2 of Hit) replaces the restatement's own mapping"""
    two, fa, one = [HEAD2], [], [HEAD1]
    total = diff = same = none = err = 0
    for n, (head, read) in enumerate(records_map_reads(reads_file, P.fmt)):
        rid = read_id(head, ">@ \t\n")
        if len(read) < P.r:
            continue
        total += 1
        h1, h2 = hits[n] if hits is not None else map_read(X, read.encode("latin-1"), P, True)
        if h1.contig != -1:
            if h2.contig != -1:
                if h1.contig != h2.contig:
                    diff += 1
                    two.append(row(rid, read, h1, ids, X.contigs) + "\t" + row(rid, read, h2, ids, X.contigs))
                    fa.append(">" + rid + "\n" + read)
                else:
                    err += 1
            else:
                same += 1
                one.append(row(rid, read, h1, ids, X.contigs))
        else:
            none += 1
    stat = "\ttotal_read_num: %d\n" % total
    for name, v in (("map_ctg_diff_num", diff), ("map_ctg_same_num", same), ("map_no_no_num", none), ("error_map_num", err)):
        stat += "\t%s: %d  %s%%\n" % (name, v, ratio(v, total))
    return {".map_reads.2ctg.gz": "\n".join(two) + "\n", ".map_reads.2ctg.gz.reads.fa.gz": "".join(q + "\n" for q in fa),
            ".map_reads.1ctg.gz": "\n".join(one) + "\n", ".map_reads.stat": stat}


def records_map_pair(path1, path2, fmt):
    """map_pair.cpp:213-266 -> [(head1, read1, head2, read2)], one entry per line the loop takes from the first file: a line
    that is no header leaves the previous pair in place, which is then mapped and counted again"""
    a, b = open_text(path1), open_text(path2)
    out = []
    i = j = 0
    head = read = head2 = read2 = ""
    mark, extra = ("@", 2) if fmt == 1 else (">", 0)

    def take(lines, at):
        return (lines[at] if at < len(lines) else ""), at + 1
    while i < len(a):
        head, i = take(a, i)
        if head[:1] == mark:
            read, i = take(a, i)
            i += extra
            head2, j = take(b, j)
            read2, j = take(b, j)
            j += extra
        out.append((head, read, head2, read2))
    return out


def run_map_pair(X, ids, file1, file2, P, hits=None):
    """hits: (n, 2, 2) -- per pair and mate the two hits of dbgk_map_reads (the second one unused)"""
    two, one, gap = [HEAD2], [HEAD1], [HEAD1]
    total = diff = same = gaps = none = 0
    delim = "@ \t" if P.fmt == 1 else "> \t"
    rid = rid2 = ""
    for n, (head, read, head2, read2) in enumerate(records_map_pair(file1, file2, P.fmt)):
        if head[:1] == delim[0]:
            rid, rid2 = read_id(head, delim), read_id(head2, delim)
        if len(read) < P.r or len(read2) < P.r:
            continue
        if hits is not None:
            h1, h2 = hits[n][0][0], hits[n][1][0]
        else:
            h1 = map_read(X, read.encode("latin-1"), P, False)[0]
            h2 = map_read(X, read2.encode("latin-1"), P, False)[0]
        total += 1
        if h1.contig != -1 and h2.contig != -1:
            line = row(rid, read, h1, ids, X.contigs) + "\t" + row(rid2, read2, h2, ids, X.contigs)
            if h1.contig != h2.contig:
                diff += 1
                two.append(line)
            else:
                same += 1
                one.append(line)
        elif h1.contig != -1 or h2.contig != -1:
            gaps += 1
            if h1.contig != -1:
                gap.append(row(rid, read, h1, ids, X.contigs))
            if h2.contig != -1:
                gap.append(row(rid2, read2, h2, ids, X.contigs))
        else:
            none += 1
    stat = "\ttotal_read_pair_num: %d\n" % total
    for name, v in (("map_ctg_diff_num", diff), ("map_ctg_same_num", same), ("map_ctg_gap_num", gaps), ("map_no_no_num", none)):
        stat += "\t%s: %d  %s%%\n" % (name, v, ratio(v, total))
    return {".map_pair.2ctg.gz": "\n".join(two) + "\n", ".map_pair.1ctg.gz": "\n".join(one) + "\n",
            ".map_pair.gap.gz": "\n".join(gap) + "\n", ".map_pair.stat": stat}


def run_case(golden_dir, case, mapper=None):
    """a golden case -> {output file name: text}; with `mapper` (reads -> hits array) the device's hits are formatted"""
    P = params_of(case["args"])
    ids, contigs = read_contig_file(os.path.join(golden_dir, case["contigs"]), P.l)
    X = Index(contigs, P.k)
    files = read_lib_file(os.path.join(golden_dir, case["lib"]))
    out = {}
    if case["program"] == "map_reads":
        for f in files:
            path = os.path.join(golden_dir, f)
            hits = None
            if mapper is not None:
                hits = mapper(X, [r.encode("latin-1") for _, r in records_map_reads(path, P.fmt)], P, True)
            for suffix, text in run_map_reads(X, ids, path, P, hits).items():
                out[os.path.basename(f) + suffix] = text
        out[case["lib"] + ".map_reads.2ctg.lib"] = "".join("OUT/%s.map_reads.2ctg.gz\n" % f for f in files)
    else:
        for f1, f2 in zip(files[0::2], files[1::2]):
            p1, p2 = os.path.join(golden_dir, f1), os.path.join(golden_dir, f2)
            hits = None
            if mapper is not None:
                recs = records_map_pair(p1, p2, P.fmt)
                flat = mapper(X, [q.encode("latin-1") for r in recs for q in (r[1], r[3])], P, False)
                hits = [(flat[2 * n], flat[2 * n + 1]) for n in range(len(recs))]
            for suffix, text in run_map_pair(X, ids, p1, p2, P, hits).items():
                out[os.path.basename(f1) + suffix] = text
        out[case["lib"] + ".map_pair.2ctg.lib"] = "".join("OUT/%s.map_pair.2ctg.gz\n" % f for f in files[0::2])
    return out


def expected_outputs(golden_dir, case):
    """{file name: text} of everything the reference wrote for a case, gz content decompressed"""
    C = os.path.join(golden_dir, case["name"])
    out = {}
    for f in sorted(os.listdir(C)):
        data = open(os.path.join(C, f), "rb").read()
        out[f] = (gzip.decompress(data) if f.endswith(".gz") else data).decode("latin-1")
    return out


NEED = [("map_reads", "2ctg"), ("map_reads", "1ctg"), ("map_reads", "map_no_no_num"), ("map_reads", "error_map_num"),
        ("map_pair", "2ctg"), ("map_pair", "1ctg"), ("map_pair", "gap"), ("map_pair", "map_no_no_num"), "dirF", "dirR",
        "ctg:ctgC_lower", "ctg:scaf", "ctg:polyA", "ctg:ctgD", "ctg:circ", "long", "len=k+s", "edge-1", "edge0", "edge1",
        "second rejected", "other letters", "key 0 only"]


def coverage(golden_dir, cases):
    """what the REFERENCE's output of the cases shows, as a set of the tags of NEED: rows per file kind, counters above zero,
    directions, contigs hit, long reads, reads of k + s - 1 / k + s / k + s + 1 bases under a small -r, a second alignment
    that was found and rejected, mapped reads with letters outside ACGTacgtNn, a read only the all-A k-mer can seed"""
    seen = set()
    for case in cases:
        P = params_of(case["args"])
        rows = {}
        for f, text in expected_outputs(golden_dir, case).items():
            if f.endswith(".stat"):
                for line in text.strip().split("\n"):
                    if int(line.split(":")[1].split()[0]) > 0:
                        seen.add((case["program"], line.split(":")[0].strip()))
            elif f.endswith("ctg.gz") or f.endswith("gap.gz"):
                for r in (q.split("\t") for q in text.split("\n")[1:] if q):
                    rows[r[0]] = r
                    seen.update([(case["program"], f.split(".")[-2]), "dir" + r[8], "ctg:" + r[4]])
                    seen.update(["long"] * (int(r[1]) > 1024) + ["len=k+s"] * (int(r[1]) == P.k + P.s))
        if case["program"] != "map_reads":
            continue
        ids, contigs = read_contig_file(os.path.join(golden_dir, case["contigs"]), P.l)
        X = Index(contigs, P.k)
        for f in read_lib_file(os.path.join(golden_dir, case["lib"])):
            for head, read in records_map_reads(os.path.join(golden_dir, f), P.fmt):
                rb, rid = read.encode("latin-1"), read_id(head, ">@ \t\n")
                if P.r < P.k + P.s and -1 <= len(rb) - P.k - P.s <= 1:
                    seen.add("edge%d" % (len(rb) - P.k - P.s))
                if rid in rows and set(read) - set("ACGTacgtNn"):
                    seen.add("other letters")
                if rid in rows and len(rb) == P.k + P.s and window_key(rb, 0, P.k)[0] == 0:
                    seen.add("key 0 only")
                h1, h2 = map_read(X, rb, P, True)
                if h1.contig != -1 and h2.contig == -1 and h2.align_len > 0:
                    seen.add("second rejected")
    return seen
