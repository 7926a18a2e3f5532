"""Python restatement of the reference's link_scaffold (link_scaffold/link_scaffold.cpp + link_func.cpp), cited line by line.
tests/golden/make_link_golden.py asserts that it equals the real program on every fixture of tests/golden/link_cases; the GPU
tests use it for inputs too large to store.

The link table is built with numpy (orient / filter / group / reduce: the part the device does); the clean-up passes and the
walk are plain loops in the reference's order."""
import gzip
import json
import os
import zipfile
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "m n i")           # -m IsMatePair, -n PairNumCut, -i InsertSize (link_func.cpp:54-55: 400, 3)
DEFAULTS = Params(m=0, n=3, i=400)

# one 2ctg line as the link stage sees it: 0-based contig index, align_contig_start / end and direction byte of each mate
PAIR_DTYPE = np.dtype([("contig1", "<i4"), ("start1", "<i4"), ("end1", "<i4"), ("contig2", "<i4"), ("start2", "<i4"),
                       ("end2", "<i4"), ("direct1", "u1"), ("direct2", "u1"), ("pad", "u1", (2,))])
LINK_DTYPE = np.dtype([("target", "<u4"), ("freq", "<u4"), ("size", "<i8")])
COUNTERS = ("FR", "RF", "FF", "RR", "wrong")
FREQ_CAP = 1023                                  # CtgLink.freq is 10 bits and stops counting there (link_func.cpp:458-463)
OUTPUTS = ("scaffold.links.all", "scaffold.links.uniq", "scaffold.pos.tab", "scaffold.seq.fa", "scaffold_repeat.seq.fa",
           "scaffold_repeat.pos.tab")


def atoi(s):
    """C atoi: leading blanks, a sign, digits; 0 when there are none"""
    s = s.lstrip(" \t\n\v\f\r")
    j = 1 if s[:1] in ("+", "-") else 0
    k = j
    while k < len(s) and s[k].isdigit() and s[k].isascii():
        k += 1
    return int(s[:k]) if k > j else 0


def split(line, delim=" \t\n"):
    out, cur = [], ""
    for ch in line:
        if ch in delim:
            if cur:
                out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur:
        out.append(cur)
    return out


def ctg_str2id(name):
    """ctgStr2Id (link_func.h:130): the number behind the first four characters"""
    return atoi(name[4:])


def read_contig_file(text):
    """read_contig_file (link_func.cpp:99-136) -> names, sequences of the contigs in file order (node 2c + 1 is contig c)"""
    names, seqs, cur = [], [], ""
    for line in text.split("\n"):
        if line[:1] == ">":
            names.append(split(line, "> \t")[0])
            if cur:
                seqs.append(cur)
            cur = ""
        else:
            cur += line
    if cur:
        seqs.append(cur)
    return names, seqs


def check_names(names):
    """the reference indexes its arrays with the number in the name; anything but 2c + 1 for contig c is undefined there"""
    for c, name in enumerate(names):
        if ctg_str2id(name) != 2 * c + 1:
            raise ValueError("contig %d is named %r: its number must be %d" % (c, name, 2 * c + 1))


def read_lib(text):
    """reading_para_file (link_func.cpp:75-95)"""
    files = []
    for line in text.split("\n"):
        if line[:1] == "#":
            continue
        t = split(line)
        if t:
            files.append(t[0])
    return files


def parse_2ctg(text, n_contigs):
    """the fields parse_pair_ends_map_file takes from every line (link_func.cpp:234-260) as PAIR_DTYPE records"""
    rows = []
    for line in text.split("\n"):
        if line[:1] == "#" or not line:
            continue
        v = split(line)
        ids = [ctg_str2id(v[4]), ctg_str2id(v[14])]
        for x in ids:
            if x % 2 != 1 or not 0 < x < 2 * n_contigs + 1:
                raise ValueError("contig id %d of a map line is no contig of the contig file" % x)
        d = [ord(t) if len(t) == 1 else ord("?") for t in (v[8], v[18])]
        rows.append((ids[0] // 2, atoi(v[6]), atoi(v[7]), ids[1] // 2, atoi(v[16]), atoi(v[17]), d[0], d[1], (0, 0)))
    return np.array(rows, dtype=PAIR_DTYPE) if rows else np.zeros(0, dtype=PAIR_DTYPE)


def orient(P, lens, recs):
    """link_func.cpp:262-313 (-m 0) and :367-415 (-m 1), 32-bit arithmetic -> src, tgt of the two directed entries of every
    record (ctg1 -> ctg3, ctg4 -> ctg2), gap, keep mask (:317, :419) and the five class counters (counted before the filter)"""
    lens = np.asarray(lens, dtype=np.int64)
    c1, c2 = recs["contig1"].astype(np.int64), recs["contig2"].astype(np.int64)
    s1, e1, s2, e2 = (recs[f].astype(np.int64) for f in ("start1", "end1", "start2", "end2"))
    f1, r1 = recs["direct1"] == ord("F"), recs["direct1"] == ord("R")
    f2, r2 = recs["direct2"] == ord("F"), recs["direct2"] == ord("R")
    FR, RF, FF, RR = f1 & r2, r1 & f2, f1 & f2, r1 & r2
    id1, id2 = 2 * c1 + 1, 2 * c2 + 1
    l1, l2 = lens[c1], lens[c2]
    n = len(recs)
    ctg1, ctg2, ctg3, ctg4, gap = (np.zeros(n, dtype=np.int64) for _ in range(5))
    I = P.i

    def put(mask, a1, a2, a3, a4, g):
        ctg1[mask], ctg2[mask], ctg3[mask], ctg4[mask], gap[mask] = a1[mask], a2[mask], a3[mask], a4[mask], g[mask]

    if P.m == 0:
        put(FR, id1, id1 + 1, id2, id2 + 1, I - (l1 - s1) - e2)                     # :262-273
        put(RF, id2, id2 + 1, id1, id1 + 1, I - (l2 - s2) - e1)                     # :274-285
        put(FF, id1, id1 + 1, id2 + 1, id2, I - (l1 - s1) - (l2 - s2))              # :286-297
        put(RR, id1 + 1, id1, id2, id2 + 1, I - (l1 - (l1 - e1)) - e2)              # :298-309
    else:
        put(FR, id2, id2 + 1, id1, id1 + 1, I - (l2 - s2) - e1)                     # :367-377
        put(RF, id1, id1 + 1, id2, id2 + 1, I - (l1 - s1) - e2)                     # :378-388
        put(FF, id1 + 1, id1, id2, id2 + 1, I - (l1 - (l1 - e1)) - e2)              # :389-400
        put(RR, id1, id1 + 1, id2 + 1, id2, I - (l1 - s1) - (l2 - s2))              # :401-411
    gap = ((gap + (1 << 31)) % (1 << 32)) - (1 << 31)                               # int gap_size
    ok = FR | RF | FF | RR
    keep = ok & (gap > -(I // 2)) & (gap <= I)                                      # -InsertSize / 2 truncates toward zero
    counters = dict(FR=int(FR.sum()), RF=int(RF.sum()), FF=int(FF.sum()), RR=int(RR.sum()), wrong=int((~ok).sum()))
    return ctg1, ctg3, ctg4, ctg2, gap, keep, counters


def build_table(P, lens, recs):
    """add_data_into_link over every kept record in record order (link_func.cpp:430-473): per node the links in first-seen order,
    each with the count and the gap sum of its first 1023 records.  -> first[n_nodes + 1], LINK_DTYPE links, counters"""
    n_nodes = 2 * len(lens) + 1
    a_src, a_tgt, b_src, b_tgt, gap, keep, counters = orient(P, lens, recs)
    idx = np.nonzero(keep)[0]
    src = np.stack([a_src[idx], b_src[idx]], axis=1).ravel()       # entry 2r: ctg1 -> ctg3, entry 2r + 1: ctg4 -> ctg2 (:319-320)
    tgt = np.stack([a_tgt[idx], b_tgt[idx]], axis=1).ravel()
    g = np.repeat(gap[idx], 2)
    key = src * n_nodes + tgt
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(len(ks), dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    starts = np.nonzero(head)[0]
    count = np.diff(np.append(starts, len(ks)))
    rank = np.arange(len(ks)) - np.repeat(starts, count)
    gs = np.where(rank < FREQ_CAP, g[order], 0)
    size = np.add.reduceat(gs, starts) if len(starts) else np.zeros(0, dtype=np.int64)
    first_seen = order[starts]
    l_src, l_tgt = src[first_seen], tgt[first_seen]
    chain = np.lexsort((first_seen, l_src))                        # a node's links in first-seen order
    links = np.zeros(len(chain), dtype=LINK_DTYPE)
    links["target"], links["freq"], links["size"] = l_tgt[chain], np.minimum(count, FREQ_CAP)[chain], size[chain]
    first = np.zeros(n_nodes + 1, dtype=np.int64)
    np.add.at(first, l_src + 1, 1)
    return np.cumsum(first), links, counters


def c_div(a, b):
    """int64 division truncated toward zero (link_func.cpp:530, :704, :833)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def pair_id(i):
    return i - 1 if i % 2 == 0 else i + 1


def fmt_float(a, b):
    """cerr << (float)a / b"""
    return "%g" % float(np.float32(a) / np.float32(b))


class Scaffolder:
    """the state main() holds behind the map files: ctgLink as lists of [id, freq, size] per node, linkStat as three lists"""

    def __init__(self, P, lens, first, links, counters):
        self.P, self.lens = P, [int(x) for x in lens]
        self.n_nodes = 2 * len(lens) + 1                                       # contig_num: node 0, contig c = node 2c + 1
        t, f, s = links["target"].tolist(), links["freq"].tolist(), links["size"].tolist()
        first = [int(x) for x in first]
        self.chain = [[[t[j], f[j], s[j]] for j in range(first[i], first[i + 1])] for i in range(self.n_nodes)]
        self.link, self.inlink, self.dele = [0] * self.n_nodes, [0] * self.n_nodes, [0] * self.n_nodes
        self.counters = dict(counters)
        self.lowfreq = self.interleave = self.deleted = 0
        self.repeat_nodes = []

    def node_len(self, i):
        return self.lens[i // 2] if i % 2 == 1 else 0                          # contig_seqs[even] is the empty string

    def remove_lowfreq_link_and_stat(self):                                    # link_func.cpp:477-511
        for i in range(self.n_nodes):
            n = 0
            for e in self.chain[i]:
                if e[1] < self.P.n:
                    e[0] = e[1] = e[2] = 0
                    self.lowfreq += 1
                else:
                    n += 1
                    if self.inlink[e[0]] < 255:
                        self.inlink[e[0]] += 1
            if self.chain[i]:
                self.link[i] = min(n, 255)

    def links_text(self):                                                      # display_data_in_link, :515-537
        out = ["ctg_id\tincoming_link_num\toutgoing_link_num\tlinked_id,pair_num,sum_size,avg_size;\n"]
        for i in range(1, self.n_nodes):
            row = "%d\t%d\t%d" % (i, self.inlink[i], self.link[i])
            for e in self.chain[i]:
                if e[1] > 0:
                    row += "\t%d,%d,%d,%d" % (e[0], e[1], e[2], c_div(e[2], e[1]))
            out.append(row + "\n")
        return "".join(out)

    def live(self, i):                                                         # get_all_linked_ids, :698-710
        return [(e[0], c_div(e[2], e[1])) for e in self.chain[i] if e[1] > 0]

    def next_linked(self, i, gap):                                             # get_next_linked_id, :826-840
        for e in self.chain[i]:
            if e[1] > 0:
                return e[0], c_div(e[2], e[1])
        return 0, gap

    def delete_linked_id(self, s, t):                                          # :671-694
        for e in self.chain[s]:
            if e[1] > 0 and e[0] == t:
                e[0] = e[1] = e[2] = 0
                if self.link[s] > 0:
                    self.link[s] -= 1
                if self.inlink[t] > 0:
                    self.inlink[t] -= 1
                break

    def remove_interleaving_links(self):                                       # :543-581
        for start in range(1, self.n_nodes):
            if self.dele[start] == 0 and self.link[start] == 2:
                lk = self.live(start)
                ids, gaps = [x[0] for x in lk], [x[1] for x in lk]
                for a, b in ((0, 1), (1, 0)):                                  # :553-564, then :566-577
                    if self.link[ids[a]] == 1 and self.inlink[ids[a]] == 1:
                        middle = ids[a] if ids[a] % 2 == 1 else ids[a] - 1
                        judge = gaps[b] * 2
                        end_node, end_insert = self.next_linked(ids[a], 0)
                        # contig_seqs[middle].size() < judge_len compares as unsigned 64-bit
                        if end_node == ids[b] and gaps[a] < judge and end_insert < judge and self.node_len(middle) < (judge & (2 ** 64 - 1)):
                            self.delete_linked_id(start, end_node)
                            self.interleave += 1

    def remove_repeat_nodes(self):                                             # :713-726
        for i in range(1, self.n_nodes):
            if self.dele[i] == 0 and (self.inlink[i] >= 2 or self.link[i] >= 2):
                self.repeat_nodes.append(i)
                self.dele[i] = 1
                self.dele[pair_id(i)] = 1
                self.repeat_nodes.append(pair_id(i))

    def remove_links_from_deleted_nodes(self):                                 # :747-785: cleared entries (target 0) are visited too
        for i in range(self.n_nodes):
            for e in self.chain[i]:
                t = e[0]
                if self.dele[i] == 1 or self.dele[t] == 1:
                    e[0] = e[1] = e[2] = 0
                    self.deleted += 1
                    if self.link[i] > 0:
                        self.link[i] -= 1
                    if self.inlink[t] > 0:
                        self.inlink[t] -= 1

    def get_linear_seq(self, start):                                           # :799-822
        out, nxt, gap = [], start, 0
        while True:
            nxt, gap = self.next_linked(nxt, gap)
            if self.dele[nxt] != 1:
                out += [gap, nxt]
            else:
                break
            self.dele[nxt] = 1
            self.dele[pair_id(nxt)] = 1
            if self.link[nxt] != 1:
                break
        return out

    def walk(self):
        """read_out_scaffold (link_scaffold.cpp:317-357) -> per scaffold the combined list: node, gap, node, ..."""
        out = []
        for i in range(1, self.n_nodes):
            if self.dele[i] == 1 or i % 2 == 0:
                continue
            self.dele[i] = 1
            self.dele[pair_id(i)] = 1
            right = self.get_linear_seq(i) if self.link[i] == 1 else []
            left = []
            if self.link[pair_id(i)] == 1:
                left = self.get_linear_seq(pair_id(i))[::-1]
                left = [pair_id(v) if k % 2 == 0 else v for k, v in enumerate(left)]
            out.append(left + [i] + right)
        return out


def std_sort(v, comp):
    """std::sort as the reference's program does it, in place.  The order it leaves equal lengths in is part of the reference's
    output (the E. coli runs have such ties), and it is that of the libstdc++ the shipped program was built with: introsort whose
    pivot is the median of first, middle and last element taken BY VALUE, partition over the whole range, ranges of up to 16
    elements left to one final insertion sort (bits/stl_algo.h of GCC 4.4; later versions move the median to the front instead
    and order some ties differently).  Found by running the three historical forms against the shipped results."""
    def linear_insert(last):
        val, nxt = v[last], last - 1
        while comp(val, v[nxt]):
            v[last] = v[nxt]
            last, nxt = nxt, nxt - 1
        v[last] = val

    def insertion_sort(first, last):
        for i in range(first + 1, last):
            if comp(v[i], v[first]):
                v[first:i + 1] = [v[i]] + v[first:i]
            else:
                linear_insert(i)

    def introsort(first, last, depth):
        while last - first > 16:
            if depth == 0:
                raise NotImplementedError("std::sort fell back to heap sort")   # (2 lg n bad pivots in a row)
            depth -= 1
            a, b, c = v[first], v[first + (last - first) // 2], v[last - 1]      # __median
            if comp(a, b):
                pivot = b if comp(b, c) else c if comp(a, c) else a
            else:
                pivot = a if comp(a, c) else c if comp(b, c) else b
            lo, hi = first, last                                                 # __unguarded_partition
            while True:
                while comp(v[lo], pivot):
                    lo += 1
                hi -= 1
                while comp(pivot, v[hi]):
                    hi -= 1
                if not lo < hi:
                    break
                v[lo], v[hi] = v[hi], v[lo]
                lo += 1
            introsort(lo, last, depth)
            last = lo

    n = len(v)
    if n:
        introsort(0, n, 2 * (n.bit_length() - 1))
        if n > 16:
            insertion_sort(0, 16)
            for i in range(16, n):
                linear_insert(i)
        else:
            insertion_sort(0, n)


def by_len(a, b):
    return b[0] < a[0]                                                          # cmpSeqByLen, link_func.cpp:69-71


def reverse_complement(seq):
    """seqKmer.cpp:72-81: N / n kept, ACGT in either case complemented to upper case, everything else N"""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "T", "c": "G", "g": "C", "t": "A", "N": "N", "n": "n"}
    return "".join(comp.get(ch, "N") for ch in reversed(seq))


def layout(scaffolds, repeat_nodes):
    """generate_scaffold (link_scaffold.cpp:427-463) as emit items: per scaffold a list of (contig, reverse) / (None, gap)"""
    out = []
    for comb in scaffolds:
        items = []
        for k, v in enumerate(comb):
            if k % 2 == 0:
                items.append((v // 2, 0) if v % 2 == 1 else ((v - 1) // 2, 1))
            else:
                items.append((None, v if v > 1 else 1))                        # the smallest gap written is 1
        out.append(items)
    return out


def emit_string(seqs, items):
    return "".join(("N" * b) if c is None else (reverse_complement(seqs[c]) if b else seqs[c]) for c, b in items)


def run(P, names, lens, recs_per_file, map_files, seqs=None, prefix="Output"):
    """main() behind option parsing -> dict: the six outputs (the two .seq.fa only with seqs), 'stderr' without the Run time lines,
    'counters', 'layout'"""
    err = []
    err.append("link_scaffold  [version 1.0]\n"
               "   -m <int>   input mapping data type: 0, pair-ends; 1. mated-pair,  default=%d\n"
               "   -n <int>   the minimum number of read pairs required to support a link between two contigs, default=%d\n"
               "   -i <int>   mean insert size for pair-ends or mated-pair reads, default=%d\n"
               "   -o <str>   the output prefix, set in commond-line, default = %s\n"
               "   -h         get the help information\n\n" % (P.m, P.n, P.i, prefix))
    err.append("\nProgram start ............\n")
    total_len = sum(int(x) for x in lens)
    err.append("\nInput contig number: %d\nInput contig length: %d\nRead contigs into memory finished !\n" % (len(lens), total_len))
    err.append("\nInput reads mapping files number: %d\n" % len(map_files))
    for f in map_files:
        err.append("\nparse map file: %s\n" % f)
    err.append("\nParsed the map files done !\n")
    recs = np.concatenate(recs_per_file) if len(recs_per_file) else np.zeros(0, dtype=PAIR_DTYPE)
    first, links, ctr = build_table(P, lens, recs)
    S = Scaffolder(P, lens, first, links, ctr)
    err.append("\nFR_link_num: %d\nRF_link_num: %d\nFF_link_num: %d\nRR_link_num: %d\nEffect_link_num: %d\nWrong_link_num: %d\n"
               % (ctr["FR"], ctr["RF"], ctr["FF"], ctr["RR"], ctr["FR"] + ctr["RF"] + ctr["FF"] + ctr["RR"], ctr["wrong"]))
    S.remove_lowfreq_link_and_stat()
    err.append("\nRemoved LowFreq link num: %d\n" % S.lowfreq)
    odd = [S.link[i] for i in range(1, S.n_nodes, 2)]
    uniq, multi, empty, total = sum(x == 1 for x in odd), sum(x > 1 for x in odd), sum(x == 0 for x in odd), len(odd)
    err.append("Number and ratio of contigs having a unique 3'-link: %d  %s\n" % (uniq, fmt_float(uniq, total)))
    err.append("Number and ratio of contigs having multiple 3'-link: %d  %s\n" % (multi, fmt_float(multi, total)))
    err.append("Number and ratio of contigs having zero 3'-link:     %d  %s\n" % (empty, fmt_float(empty, total)))
    out = {"scaffold.links.all": S.links_text()}
    S.remove_interleaving_links()
    err.append("\nRemoved interleave links num: %d\n" % S.interleave)
    S.remove_repeat_nodes()
    err.append("\nRemoved repeat nodes num: %d\n" % (len(S.repeat_nodes) // 2))
    S.remove_links_from_deleted_nodes()
    err.append("\nRemoved links [related with repeat or small nodes] num: %d\n" % S.deleted)
    out["scaffold.links.uniq"] = S.links_text()

    scaffolds = S.walk()
    lay = layout(scaffolds, S.repeat_nodes)
    rows = []                                                                  # link_scaffold.cpp:366-406
    tot_num = tot_len = tot_wogap = inc_num = inc_len = 0
    for w, items in enumerate(lay):
        pos, scaf_len, wogap, n_ctg = "", 0, 0, 0
        for c, b in items:
            if c is not None:
                n_ctg += 1
                size = int(lens[c])
                pos += "\t%s\t%d\t%d\t%d\t%s\n" % (names[c], scaf_len + 1, scaf_len + size, size, "R" if b else "F")
                scaf_len += size
                wogap += size
                inc_num += 1
                inc_len += size
            else:
                pos += "\tgap\t%d\t%d\t%d\tN\n" % (scaf_len + 1, scaf_len + b, b)
                scaf_len += b
        head = "   fragment_num:%d   length:%d   lenwogap:%d\n" % (n_ctg, scaf_len, wogap)
        rows.append((scaf_len, w, head, pos, items))
        tot_num += 1
        tot_len += scaf_len
        tot_wogap += wogap
    std_sort(rows, by_len)
    scaffold_id = -1
    pos_tab, seq_fa = [], []
    for scaf_len, w, head, pos, items in rows:
        scaffold_id += 2
        pos_tab.append(">scf_%d\n%s" % (scaffold_id, pos))
        if seqs is not None:
            seq_fa.append(">scf_%d%s%s\n" % (scaffold_id, head, emit_string(seqs, items)))
    out["scaffold.pos.tab"] = "".join(pos_tab)
    if seqs is not None:
        out["scaffold.seq.fa"] = "".join(seq_fa)

    rep = [(int(lens[v // 2]), v // 2) for v in S.repeat_nodes if v % 2 == 1]   # link_scaffold.cpp:253-275
    exc_num, exc_len = len(rep), sum(r[0] for r in rep)
    std_sort(rep, by_len)
    rpos, rseq = [], []
    for size, c in rep:
        scaffold_id += 2
        rpos.append(">scf_%d\n\t%s\t1\t%d\t%d\tF\n" % (scaffold_id, names[c], size, size))
        if seqs is not None:
            rseq.append(">scf_%d   fragment_num:1   length:%d   lenwogap:%d   RepeatNode\n%s\n" % (scaffold_id, size, size, seqs[c]))
    out["scaffold_repeat.pos.tab"] = "".join(rpos)
    if seqs is not None:
        out["scaffold_repeat.seq.fa"] = "".join(rseq)

    err.append("\nRead out scaffold sequence done\n")
    err.append("\nTotal scaffold number:          %d\nTotal scaffold length[WithGap]: %d\nTotal scaffold length[NoGap]:   %d\n"
               % (tot_num, tot_len, tot_wogap))
    err.append("\nIncluded contig number: %d  %s\n" % (inc_num, fmt_float(inc_num, len(lens))))
    err.append("Included contig length: %d  %s\n" % (inc_len, fmt_float(inc_len, total_len)))
    err.append("Excluded repeat contig number: %d  %s\n" % (exc_num, fmt_float(exc_num, len(lens))))
    err.append("Excluded repeat contig length: %d  %s\n" % (exc_len, fmt_float(exc_len, total_len)))
    err.append("\nProgram finished !\n")
    out["stderr"] = "".join(err)
    out["counters"] = dict(ctr, lowfreq=S.lowfreq, interleave=S.interleave, repeat=len(S.repeat_nodes) // 2, deleted=S.deleted,
                           scaffolds=tot_num)
    out["layout"] = [r[4] for r in rows]
    return out


# ---- the fixtures of tests/golden/link_cases -----------------------------------------------------------------------------

def strip_run_time(text):
    return "".join(l for l in text.splitlines(True) if not l.startswith("Run time:"))


def case_params(case):
    a = case["args"]
    get = lambda flag, d: int(a[a.index(flag) + 1]) if flag in a else d  # noqa: E731
    return Params(m=get("-m", DEFAULTS.m), n=get("-n", DEFAULTS.n), i=get("-i", DEFAULTS.i))


def case_files(D, case):
    """a fixture is one archive <case>.zip: its inputs, and expected/ with what the reference wrote -> {member name: bytes}"""
    with zipfile.ZipFile(os.path.join(D, case["name"] + ".zip")) as z:
        return {n: z.read(n) for n in z.namelist()}


def unpack_inputs(D, case, dest):
    """the inputs of a fixture as files in dest, for the command line"""
    os.makedirs(dest, exist_ok=True)
    for n, d in case_files(D, case).items():
        if not n.startswith("expected/"):
            open(os.path.join(dest, n), "wb").write(d)


def load_case(D, case):
    """-> P, names, lens, seqs (None for a lengths-only case), records per map file, map file names as the .lib gives them"""
    F = case_files(D, case)
    if "lengths" in case:
        rows = [line.split() for line in F[case["lengths"]].decode().splitlines() if line.strip()]
        names, lens, seqs = [t[0] for t in rows], [int(t[1]) for t in rows], None
    else:
        names, seqs = read_contig_file(F[case["contigs"]].decode("latin-1"))
        lens = [len(q) for q in seqs]
    check_names(names)
    files = read_lib(F[case["lib"]].decode())
    recs = [parse_2ctg(gzip.decompress(F[f]).decode("latin-1"), len(names)) for f in files]
    return case_params(case), names, lens, seqs, recs, files


def output_name(case, P, kind):
    return "%s.insert%d.%s" % (case["prefix"], P.i, kind)


def expected_outputs(D, case):
    return {n[len("expected/"):]: d.decode("latin-1") for n, d in sorted(case_files(D, case).items()) if n.startswith("expected/")}


def run_case(D, case):
    """the restatement on one fixture -> {file name: text} named as expected_outputs names them"""
    P, names, lens, seqs, recs, files = load_case(D, case)
    res = run(P, names, lens, recs, files, seqs, prefix=case["prefix"])
    got = {output_name(case, P, k): res[k] for k in OUTPUTS if k in res}
    got["stderr.txt"] = res["stderr"]
    return got, res


def split_records(text):
    """a pos.tab or seq.fa text as a sorted list of records with their scaffold ids blanked (the tie case)"""
    recs = [r.split("\n", 1) for r in text.split(">scf_") if r]
    return sorted((h.lstrip("0123456789"), b) for h, b in recs)


def golden_cases(D):
    return json.load(open(os.path.join(D, "cases.json")))
