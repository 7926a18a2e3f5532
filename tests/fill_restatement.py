"""Python restatement of the reference's link_contig (link_scaffold/link_contig.cpp + link_func.cpp), cited line by line.
tests/golden/make_fill_golden.py asserts that it equals the real program on every fixture of tests/golden/fill_cases; the GPU
tests use it for inputs too large to store.  The passes, the walk and the pinned std::sort are those of link_restatement.py."""
import gzip
import json
import os
from collections import namedtuple

import numpy as np

import link_restatement as LR

Params = namedtuple("Params", "n")               # -n PairNumCut (link_func.cpp:55: 3)
DEFAULTS = Params(n=3)

# one 2ctg line as link_contig sees it: read index, fields 1, 3, 12, 0-based contig indices of fields 4 and 14, direction bytes
REC_DTYPE = np.dtype([("read", "<i4"), ("read_len", "<i4"), ("align1_end", "<i4"), ("align2_start", "<i4"), ("contig1", "<i4"),
                      ("contig2", "<i4"), ("direct1", "u1"), ("direct2", "u1"), ("pad", "u1", (2,))])
OUTPUTS = ("contig_R.links.all", "contig_R.links.uniq", "contig_R.seq.fa", "contig_R.pos.tab", "contig_R.repeat.seq.fa",
           "contig_R.repeat.pos.tab")
POS_HEADER = ("#scafftig_id\tblock_id\tblock_start\tblock_end\tblock_size\tdirection\tgapsize_mode_freq\tgapsize_total_freq\t"
              "gapsize_variance\tgapseq_identity\n")


def wrap32(x):
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def parse_2ctg(text, n_contigs, read_index):
    """the fields of parse_read_ends_map_file (link_func.cpp:167-173) and load_map_twoctg_file (link_contig.cpp:633-642);
    read_index: read id -> index, extended in the order the lines name new ids"""
    rows = []
    for line in text.split("\n"):
        if line[:1] == "#" or not line:
            continue
        v = LR.split(line)
        ids = [LR.ctg_str2id(v[4]), LR.ctg_str2id(v[14])]
        for x in ids:
            if x % 2 != 1 or not 0 < x < 2 * n_contigs + 1:
                raise ValueError("contig id %d of a map line is no contig of the contig file" % x)
        d = [ord(t) if len(t) == 1 else ord("?") for t in (v[8], v[18])]
        r = read_index.setdefault(v[0], len(read_index))
        rows.append((r, LR.atoi(v[1]), LR.atoi(v[3]), LR.atoi(v[12]), ids[0] // 2, ids[1] // 2, d[0], d[1], (0, 0)))
    return np.array(rows, dtype=REC_DTYPE) if rows else np.zeros(0, dtype=REC_DTYPE)


def load_reads(text, read_index, seqs):
    """load_reads_fa_file (link_contig.cpp:651-672): a later entry of an id replaces an earlier one"""
    lines = text.split("\n")
    k = 0
    while k < len(lines):
        if lines[k][:1] == ">":
            t = LR.split(lines[k], "> \t\n")
            seq = lines[k + 1] if k + 1 < len(lines) else ""
            k += 1
            if t and t[0] in read_index:
                seqs[read_index[t[0]]] = seq
        k += 1


def gaps_of(recs):
    return wrap32(recs["align2_start"].astype(np.int64) - recs["align1_end"].astype(np.int64) - 1)


def build_table(recs, n_contigs):
    """parse_read_ends_map_file (link_func.cpp:175-217) + add_data_into_link (:430-473): FF, RR, FR, RF give ctg1 -> ctg3 and
    ctg4 -> ctg2, no gap filter; per node the links in first-seen order, count and gap sum of the first 1023 records"""
    n_nodes = 2 * n_contigs + 1
    f1, r1 = recs["direct1"] == ord("F"), recs["direct1"] == ord("R")
    f2, r2 = recs["direct2"] == ord("F"), recs["direct2"] == ord("R")
    FR, RF, FF, RR = f1 & r2, r1 & f2, f1 & f2, r1 & r2
    ok = FR | RF | FF | RR
    counters = dict(FR=int(FR.sum()), RF=int(RF.sum()), FF=int(FF.sum()), RR=int(RR.sum()), wrong=int((~ok).sum()))
    id1, id2 = 2 * recs["contig1"].astype(np.int64) + 1, 2 * recs["contig2"].astype(np.int64) + 1
    ctg1, ctg2 = id1 + r1, id1 + f1
    ctg3, ctg4 = id2 + r2, id2 + f2
    gap = gaps_of(recs)
    idx = np.nonzero(ok)[0]
    src = np.stack([ctg1[idx], ctg4[idx]], axis=1).ravel()
    tgt = np.stack([ctg3[idx], ctg2[idx]], axis=1).ravel()
    g = np.repeat(gap[idx], 2)
    key = src * n_nodes + tgt
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(len(ks), dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    starts = np.nonzero(head)[0]
    count = np.diff(np.append(starts, len(ks)))
    rank = np.arange(len(ks)) - np.repeat(starts, count)
    gs = np.where(rank < LR.FREQ_CAP, g[order], 0)
    size = np.add.reduceat(gs, starts) if len(starts) else np.zeros(0, dtype=np.int64)
    first_seen = order[starts]
    l_src, l_tgt = src[first_seen], tgt[first_seen]
    chain = np.lexsort((first_seen, l_src))
    links = np.zeros(len(chain), dtype=LR.LINK_DTYPE)
    links["target"], links["freq"], links["size"] = l_tgt[chain], np.minimum(count, LR.FREQ_CAP)[chain], size[chain]
    first = np.zeros(n_nodes + 1, dtype=np.int64)
    np.add.at(first, l_src + 1, 1)
    return np.cumsum(first), links, counters


def gap_stats(recs):
    """decide_gap_size (link_contig.cpp:569-610) per unordered contig pair, records of every direction pooled
    -> {(lo, hi): (mode, mode_freq, total_freq, variance, indices of the records whose gap is the mode, in file order)}"""
    lo = np.minimum(recs["contig1"], recs["contig2"]).astype(np.int64)
    hi = np.maximum(recs["contig1"], recs["contig2"]).astype(np.int64)
    gap = gaps_of(recs)
    order = np.lexsort((gap, hi, lo))              # stable: file order within (pair, gap)
    out = {}
    if not len(recs):
        return out
    klo, khi, kg = lo[order], hi[order], gap[order]
    new_run = np.ones(len(order), dtype=bool)
    new_run[1:] = (klo[1:] != klo[:-1]) | (khi[1:] != khi[:-1]) | (kg[1:] != kg[:-1])
    rs = np.nonzero(new_run)[0]
    re = np.append(rs[1:], len(order))
    cur, runs = None, []

    def close():
        mode, mode_freq, at = 0, 0, None
        for g, a, b in runs:                       # ascending map<int,int>, strict >
            if b - a > mode_freq:
                mode, mode_freq, at = g, b - a, (a, b)
        total = sum(b - a for _, a, b in runs)
        var = 0
        for g, a, b in runs:
            var = int(wrap32(var + int(wrap32(abs(int(wrap32(g - mode))) * (b - a)))))
        out[cur] = (mode, mode_freq, total, LR.c_div(var, total), order[at[0]:at[1]])

    for a, b in zip(rs.tolist(), re.tolist()):
        k = (int(klo[a]), int(khi[a]))
        if k != cur:
            if cur is not None:
                close()
            cur, runs = k, []
        runs.append((int(kg[a]), a, b))
    close()
    return out


def rev_com_seq(seq):
    return LR.reverse_complement(seq)              # seqKmer.cpp:83-91, the same table as reverse_complement


def consensus(slices):
    """link_contig.cpp:488-510 -> consensus string, per-column consensus_freq, support rate (float, column 0 first)"""
    gap = len(slices[0])
    cons, freqs = [], []
    rate = np.float32(0.0)
    for k in range(gap):
        stat = {}
        for s in slices:
            stat[s[k]] = stat.get(s[k], 0) + 1
        best, bf = None, 0
        for ch in sorted(stat, key=lambda c: ord(c) if ord(c) < 128 else ord(c) - 256):   # ascending map<char,int>, strict >
            if stat[ch] > bf:
                best, bf = ch, stat[ch]
        cons.append(best)
        freqs.append(bf)
        rate = np.float32(rate + np.float32(np.float32(bf) / np.float32(len(slices))))
    rate = np.float32(rate / np.float32(gap))
    return "".join(cons), freqs, rate


def float9(x):
    """boost::lexical_cast<string>(float)"""
    return "%.9g" % float(np.float32(x))


def fill(scaffolds, lens, recs, stats, reads=None):
    """fill_gaps_inside_scaffold (link_contig.cpp:372-551) without the strings -> per scafftig a list of items
    ('ctg', contig, reversed, length) / ('gap', mode, mode_freq, total_freq, variance, consensus or None, identity or None)"""
    out = []
    for comb in scaffolds:
        items = []
        for j in range(0, len(comb), 2):
            v = comb[j]
            c, rev = (v // 2, 0) if v % 2 == 1 else ((v - 1) // 2, 1)
            if j + 2 >= len(comb):
                items.append(("ctg", c, rev, int(lens[c])))
                break
            v2 = comb[j + 2]
            c2, rev2 = (v2 // 2, 0) if v2 % 2 == 1 else ((v2 - 1) // 2, 1)
            mode, mf, tf, var, span = stats[(min(c, c2), max(c, c2))]
            if mode <= 0:
                keep = int(lens[c]) + mode             # substr(0, negative) keeps the whole contig (:441)
                items.append(("ctg", c, rev, keep if keep >= 0 else int(lens[c])))
                items.append(("gap", mode, mf, tf, var, None, None))
            else:
                items.append(("ctg", c, rev, int(lens[c])))
                cons = ident = None
                if reads is not None:
                    slices = []
                    for r in span.tolist():
                        rec = recs[r]
                        a = int(rec["align1_end"])
                        s = reads[int(rec["read"])]
                        if a < 0 or a + mode > len(s):
                            raise ValueError("a spanning read is shorter than its slice")
                        s = s[a:a + mode]
                        d1, c1 = chr(int(rec["direct1"])), int(rec["contig1"])
                        if (c1 == c and d1 != "FR"[rev]) or (c1 == c2 and d1 != "FR"[rev2]):   # :481
                            s = rev_com_seq(s)
                        slices.append(s)
                    cons, _, ident = consensus(slices)
                items.append(("gap", mode, mf, tf, var, cons, ident))
        out.append(items)
    return out


def item_len(it):
    return it[3] if it[0] == "ctg" else max(it[1], 0)


def emit_string(seqs, items):
    out = []
    for it in items:
        if it[0] == "ctg":
            s = LR.reverse_complement(seqs[it[1]]) if it[2] else seqs[it[1]]
            out.append(s[:it[3]])
        elif it[1] > 0:
            out.append(it[5])
    return "".join(out)


def run(P, names, lens, recs_per_file, map_files, seqs=None, reads=None, prefix="Output"):
    """main() behind option parsing -> dict: the six outputs (sequences only with seqs and reads), 'stderr' without the Run time
    lines, 'counters', 'layout' (items per scafftig in output order), 'stats', 'table'"""
    err = ["link_scafftig   [version 1.0]\n"
           "   -n <int>   the minimum number of read-ends required to support a link between two contigs, default=%d\n"
           "   -o <str>   the output prefix, set in commond-line, default = %s\n"
           "   -h         get the help information\n\n" % (P.n, prefix)]
    err.append("\nProgram start ............\n")
    total_len = sum(int(x) for x in lens)
    err.append("\nInput contig number: %d\nInput contig length: %d\nRead contigs into memory finished !\n" % (len(lens), total_len))
    err.append("\nInput reads mapping files number: %d\n" % len(map_files))
    for f in map_files:
        err.append("\nparse map file: %s\n" % f)
    err.append("\nParsed the map files done !\n")
    recs = np.concatenate(recs_per_file) if len(recs_per_file) else np.zeros(0, dtype=REC_DTYPE)
    first, links, ctr = build_table(recs, len(lens))
    S = LR.Scaffolder(LR.Params(0, P.n, 1), lens, first, links, ctr)
    err.append("\nFR_link_num: %d\nRF_link_num: %d\nFF_link_num: %d\nRR_link_num: %d\nEffect_link_num: %d\nWrong_link_num: %d\n"
               % (ctr["FR"], ctr["RF"], ctr["FF"], ctr["RR"], ctr["FR"] + ctr["RF"] + ctr["FF"] + ctr["RR"], ctr["wrong"]))
    S.remove_lowfreq_link_and_stat()
    err.append("\nRemoved LowFreq link num: %d\n" % S.lowfreq)
    odd = [S.link[i] for i in range(1, S.n_nodes, 2)]
    uniq, multi, empty, total = sum(x == 1 for x in odd), sum(x > 1 for x in odd), sum(x == 0 for x in odd), len(odd)
    err.append("Number and ratio of contigs having a unique 3'-link: %d  %s\n" % (uniq, LR.fmt_float(uniq, total)))
    err.append("Number and ratio of contigs having multiple 3'-link: %d  %s\n" % (multi, LR.fmt_float(multi, total)))
    err.append("Number and ratio of contigs having zero 3'-link:     %d  %s\n" % (empty, LR.fmt_float(empty, total)))
    out = {"contig_R.links.all": S.links_text()}
    S.remove_repeat_nodes()
    err.append("\nRemoved repeat nodes num: %d\n" % (len(S.repeat_nodes) // 2))
    S.remove_links_from_deleted_nodes()
    err.append("\nRemoved links [related with repeat or small nodes] num: %d\n" % S.deleted)
    out["contig_R.links.uniq"] = S.links_text()
    scaffolds = S.walk()                                                       # read_out_scaffinfo, link_contig.cpp:676-726
    for f in map_files:
        err.append("\nparse reads file: %s.reads.fa.gz\n" % f)
    err.append("load reads used to fill gaps done\n\n")
    for f in map_files:
        err.append("\nparse reads file: %s\n" % f)
    err.append("load reads mapping results done\n\n")
    stats = gap_stats(recs)
    err.append("Decide the gap sizes done\n\n")
    lay = fill(scaffolds, lens, recs, stats, reads)
    rows = []
    tot_len = inc_num = inc_len = 0
    for w, items in enumerate(lay):
        pos, at, n_ctg = "", 0, 0
        for it in items:
            if it[0] == "ctg":
                n_ctg += 1
                pos += "\t%s\t%d\t%d\t%d\t%s\n" % (names[it[1]], at + 1, at + it[3], it[3], "R" if it[2] else "F")
                at += it[3]
                inc_num += 1
                inc_len += it[3]
            elif it[1] <= 0:
                pos += "\tgap\t%d\t%d\t%d\tN\t%d\t%d\t%d\n" % (at, at, it[1], it[2], it[3], it[4])
            else:
                pos += "\tgap\t%d\t%d\t%d\tN\t%d\t%d\t%d\t%s\n" % (at + 1, at + it[1], it[1], it[2], it[3], it[4],
                                                                  float9(it[6]) if it[6] is not None else "?")
                at += it[1]
        head = "   fragment_num:%d   length:%d   lenwogap:%d\n" % (n_ctg, at, at)
        rows.append((at, w, head, pos, items))
        tot_len += at
    LR.std_sort(rows, LR.by_len)
    sid = -1
    pos_tab, seq_fa = [POS_HEADER], []
    full = seqs is not None and reads is not None
    for at, w, head, pos, items in rows:
        sid += 2
        pos_tab.append(">sct_%d\n%s" % (sid, pos))
        if full:
            seq_fa.append(">sct_%d%s%s\n" % (sid, head, emit_string(seqs, items)))
    out["contig_R.pos.tab"] = "".join(pos_tab)
    if full:
        out["contig_R.seq.fa"] = "".join(seq_fa)
    err.append("Fill all gaps done\n\n")
    err.append("\nFill gaps inside scaffold sequence done\n")
    rep = [(int(lens[v // 2]), v // 2) for v in S.repeat_nodes if v % 2 == 1]
    exc_num, exc_len = len(rep), sum(r[0] for r in rep)
    LR.std_sort(rep, LR.by_len)
    rpos, rseq = [], []
    for size, c in rep:
        sid += 2
        rpos.append(">sct_%d\n\t%s\t1\t%d\t%d\tF\n" % (sid, names[c], size, size))
        if seqs is not None:
            rseq.append(">sct_%d   fragment_num:1   length:%d   lenwogap:%d   RepeatNode\n%s\n" % (sid, size, size, seqs[c]))
    out["contig_R.repeat.pos.tab"] = "".join(rpos)
    if seqs is not None:
        out["contig_R.repeat.seq.fa"] = "".join(rseq)
    err.append("\nTotal scafftig number:          %d\nTotal scafftig length[WithGap]: %d\nTotal scafftig length[NoGap]:   %d\n"
               % (len(rows), tot_len, tot_len))
    err.append("\nIncluded contig number: %d  %s\n" % (inc_num, LR.fmt_float(inc_num, len(lens))))
    err.append("Included contig length: %d  %s\n" % (inc_len, LR.fmt_float(inc_len, total_len)))
    err.append("Excluded repeat contig number: %d  %s\n" % (exc_num, LR.fmt_float(exc_num, len(lens))))
    err.append("Excluded repeat contig length: %d  %s\n" % (exc_len, LR.fmt_float(exc_len, total_len)))
    err.append("\nProgram finished !\n")
    out["stderr"] = "".join(err)
    out["counters"] = dict(ctr, lowfreq=S.lowfreq, repeat=len(S.repeat_nodes) // 2, deleted=S.deleted, scaffolds=len(rows))
    out["layout"] = [r[4] for r in rows]
    out["repeats"] = [c for _, c in rep]
    out["stats"] = stats
    out["table"] = (first, links, ctr)
    return out


# ---- the fixtures of tests/golden/fill_cases -----------------------------------------------------------------------------

def case_params(case):
    a = case["args"]
    return Params(n=int(a[a.index("-n") + 1]) if "-n" in a else DEFAULTS.n)


def load_case(D, case):
    """-> P, names, seqs, records per map file, map file names, reads (list by read index)"""
    F = LR.case_files(D, case)
    names, seqs = LR.read_contig_file(F[case["contigs"]].decode("latin-1"))
    LR.check_names(names)
    files = LR.read_lib(F[case["lib"]].decode())
    index = {}
    recs = [parse_2ctg(gzip.decompress(F[f]).decode("latin-1"), len(names), index) for f in files]
    reads = [""] * len(index)
    for f in files:
        load_reads(gzip.decompress(F[f + ".reads.fa.gz"]).decode("latin-1"), index, reads)
    return case_params(case), names, seqs, recs, files, reads


def run_case(D, case):
    P, names, seqs, recs, files, reads = load_case(D, case)
    res = run(P, names, [len(s) for s in seqs], recs, files, seqs, reads, prefix=case["prefix"])
    got = {"%s.%s" % (case["prefix"], k): res[k] for k in OUTPUTS}
    got["stderr.txt"] = res["stderr"]
    return got, res


def split_records(text):
    """a pos.tab or seq.fa text as a sorted list of records with their scafftig ids blanked (the tie case)"""
    recs = [r.split("\n", 1) for r in text.split(">sct_") if r]
    return sorted((h.lstrip("0123456789"), b) for h, b in recs)


def compare_outputs(case, got, want):
    """byte for byte; a case with a length tie as a multiset of records with their ids blanked when its order is not pinned"""
    assert sorted(got) == sorted(want)
    for f in sorted(want):
        assert got[f] == want[f], f


def golden_cases(D):
    return json.load(open(os.path.join(D, "cases.json")))
