"""Python restatement of the reference's link_supertig (link_scaffold/link_supertig.cpp + link_func.cpp), cited line by line.
tests/golden/make_super_golden.py asserts that it equals the real program on every fixture of tests/golden/super_cases; the GPU
tests use it for inputs too large to store.  The table is fill_restatement's, the passes, the walk and the pinned std::sort are
those of link_restatement.py."""
import gzip
import json
import os
from collections import namedtuple

import numpy as np

import fill_restatement as FR
import link_restatement as LR

Params = namedtuple("Params", "n")               # -n PairNumCut (link_func.cpp:55: 3)
DEFAULTS = Params(n=3)
REC_DTYPE = FR.REC_DTYPE
OUTPUTS = ("supertig.links.all", "supertig.links.uniq", "supertig.seq.fa", "supertig.pos.tab", "supertig.gap.data",
           "supertig_repeat.seq.fa", "supertig_repeat.pos.tab")
SIDE = 250                                       # side_extend_len, link_supertig.cpp:454


class BadSlice(ValueError):
    """the reference throws out of substr here (:457) and aborts"""

    def __init__(self, record, read, left, right):
        ValueError.__init__(self, "record %d: read %d over contigs %d / %d has no slice" % (record, read, left, right))
        self.record, self.read, self.left, self.right = record, read, left, right


def usage_text(n=3, prefix="Output"):
    return ("\nlink_supertig  <contig|scafftig_file.fa>  <mapping_twoctg_files.lib>\n"
            "   Function: link illumina-derived scafftigs into super-contigs by pacbio reads, inside gap are filled\n"
            "   Version: 1.0\n"
            "   -n <int>   the minimum number of read-ends required to support a link, default=%d\n"
            "   -o <str>   the output prefix, set in commond-line, default = %s\n"
            "   -h         get the help information\n\n"
            "Example:    link_supertig Ecoli.scafftig.seq.fa  pacbio_mapping.lib\n\n" % (n, prefix))


def trunc_mean(total, n):
    """int / int of C: toward zero (gaps -3 and -4 give -3)"""
    return LR.c_div(int(total), int(n))


def gap_stats(recs):
    """decide_gap_size (link_supertig.cpp:561-605) per unordered contig pair, records of every direction pooled, in file order
    -> {(lo, hi): (mean, min, max, total, variance, indices of the pair's records in file order)}"""
    lo = np.minimum(recs["contig1"], recs["contig2"]).astype(np.int64)
    hi = np.maximum(recs["contig1"], recs["contig2"]).astype(np.int64)
    gap = FR.gaps_of(recs)
    out = {}
    if not len(recs):
        return out
    order = np.lexsort((hi, lo))                   # stable: file order within a pair
    klo, khi = lo[order], hi[order]
    new = np.ones(len(order), dtype=bool)
    new[1:] = (klo[1:] != klo[:-1]) | (khi[1:] != khi[:-1])
    starts = np.nonzero(new)[0]
    ends = np.append(starts[1:], len(order))
    for a, b in zip(starts.tolist(), ends.tolist()):
        idx = order[a:b]
        g = gap[idx]
        total = b - a
        s = int(g.sum())
        if not -(1 << 31) <= s < (1 << 31):
            raise OverflowError("the gap sum of a pair leaves int")
        mean = trunc_mean(s, total)
        dev = int(np.abs(mean - g).sum())
        if dev >= (1 << 31):
            raise OverflowError("the deviation sum of a pair leaves int")
        out[(int(klo[a]), int(khi[a]))] = (mean, int(g.min()), int(g.max()), total, trunc_mean(dev, total), idx)
    return out


def slice_geometry(align1_end, align2_start, read_len):
    """link_supertig.cpp:452-457 -> (pos, len) of read.substr, or None where substr throws (read_len None: no such read)"""
    g = align2_start - align1_end - 1 if align2_start > align1_end else 0
    mid = LR.c_div(align1_end + align2_start, 2)
    pos = mid - SIDE - LR.c_div(g, 2)
    if read_len is None or pos < 0 or pos > read_len:
        return None
    return pos, min(g + 2 * SIDE, read_len - pos)


def median_index(n):
    return n // 2                                  # :470


def keeps(length, median_len):
    """:484, size_t against double"""
    return float(length) > float(median_len) * 0.75 and float(length) < float(median_len) * 1.25


def junction(recs, idx, c, rev, c2, rev2, reads):
    """:443-495 for one gap -> dict: slices as sorted (length, record, reversed, kept 2 median / 1 written / 0 dropped, bytes or None),
    median index"""
    rows = []
    for k, r in enumerate(idx.tolist()):
        rec = recs[r]
        read = int(rec["read"])
        seq = reads[read] if 0 <= read < len(reads) else None
        geo = slice_geometry(int(rec["align1_end"]), int(rec["align2_start"]), None if seq is None else len(seq))
        if geo is None:
            raise BadSlice(r, read, c, c2)
        d1, c1 = chr(int(rec["direct1"])), int(rec["contig1"])
        flip = (c1 == c and d1 != "FR"[rev]) or (c1 == c2 and d1 != "FR"[rev2])       # :459
        rows.append((geo[1], k, r, geo[0], 1 if flip else 0))
    LR.std_sort(rows, LR.by_len)                   # :469
    m = median_index(len(rows))
    mlen = rows[m][0]
    out = []
    for k, (length, _, r, pos, flip) in enumerate(rows):
        kept = 2 if k == m else 1 if keeps(length, mlen) else 0
        data = None
        if kept:
            data = reads[int(recs[r]["read"])][pos:pos + length]
            if flip:
                data = FR.rev_com_seq(data)
        out.append((length, r, flip, kept, data))
    return {"slices": out, "median": m}


def run(P, names, lens, recs_per_file, map_files, seqs=None, reads=None, prefix="Output"):
    """main() behind option parsing -> dict: the seven outputs (sequences only with seqs), 'stderr' without the Run time lines,
    'counters', 'layout' (items per super-contig in output order), 'junctions' (walk order), 'stats', 'table'.
    reads: list by read index, None for a read no reads file holds."""
    err = ["link_supertig   [version 1.0]\n"
           "   -n <int>   the minimum number of read-ends required to support a link, default=%d\n"
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
    first, links, ctr = FR.build_table(recs, len(lens))
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
    out = {"supertig.links.all": S.links_text()}
    S.remove_interleaving_links()                  # link_supertig.cpp:206
    err.append("\nRemoved interleave links num: %d\n" % S.interleave)
    S.remove_repeat_nodes()
    err.append("\nRemoved repeat nodes num: %d\n" % (len(S.repeat_nodes) // 2))
    S.remove_links_from_deleted_nodes()
    err.append("\nRemoved links [related with repeat or small nodes] num: %d\n" % S.deleted)
    out["supertig.links.uniq"] = S.links_text()
    scaffolds = S.walk()                           # read_out_scaffinfo, :671-721
    for f in map_files:
        err.append("\nparse reads file: %s.reads.fa.gz\n" % f)
    err.append("load reads used to fill gaps done\n\n")
    for f in map_files:
        err.append("\nparse map file: %s\n" % f)
    err.append("load reads mapping results done\n\n")
    stats = gap_stats(recs)
    err.append("Decide the gap sizes done\n\n")
    # fill_gaps_inside_scaffold, :364-541
    rows, junctions, gap_data = [], [], []
    gap_id, s_id = 1, 1
    tot_len = inc_num = inc_len = 0
    for w, comb in enumerate(scaffolds):
        items, pos, at, n_ctg = [], "", 0, 0
        for j in range(0, len(comb), 2):
            v = comb[j]
            c, rev = (v // 2, 0) if v % 2 == 1 else ((v - 1) // 2, 1)
            size = int(lens[c])
            n_ctg += 1
            items.append(("ctg", c, rev, size))
            oriented = "" if seqs is None else (LR.reverse_complement(seqs[c]) if rev else seqs[c])
            pos += "\t%s\t%d\t%d\t%d\t%s\t%s\n" % (names[c], at + 1, at + size, size, "R" if rev else "F", oriented)
            at += size
            inc_num += 1
            inc_len += size
            if j + 2 >= len(comb):
                break
            v2 = comb[j + 2]
            c2, rev2 = (v2 // 2, 0) if v2 % 2 == 1 else ((v2 - 1) // 2, 1)
            mean, mn, mx, tf, var, idx = stats[(min(c, c2), max(c, c2))]
            written = mean
            if mean <= 0:                          # :430-433
                written = 1
                err.append("Error may happens: mean_gap_size <= 0\n")
            J = {"gap_id": gap_id, "left": c, "right": c2, "stats": (mean, mn, mx, tf, var), "written": written, "slices": None}
            if reads is not None:
                J.update(junction(recs, idx, c, rev, c2, rev2, reads))
                sl = J["slices"]
                med = sl[J["median"]]
                body = "Y\tS%d\t+\t0\t%d\t%s\n" % (s_id, med[0], med[4])
                s_id += 1
                nodes = 1
                for k, (length, _, _, kept, data) in enumerate(sl):
                    if k == J["median"]:
                        continue
                    if kept:
                        body += "N\tS%d\t+\t0\t%d\t%s\n" % (s_id, length, data)
                        s_id += 1
                        nodes += 1
                    else:
                        err.append("Altert message:  gap_id %d  %d\t%d\n" % (gap_id, med[0], length))
                gap_data.append(">gap%d length=%d nodes=%d\n%s" % (gap_id, med[0], nodes, body))
            junctions.append(J)
            items.append(("gap", gap_id, written, mn, mx, tf, var, mean))
            pos += "\tgap%d\t%d\t%d\t%d\tN\t%d\t%d\t%d\t%d\n" % (gap_id, at + 1, at + written, written, mn, mx, tf, var)
            at += written
            gap_id += 1
        head = "   fragment_num:%d   length:%d   lenwogap:%d\n" % (n_ctg, at, at)
        rows.append((at, w, head, pos, items))
        tot_len += at
    LR.std_sort(rows, LR.by_len)                   # :544
    sid = -1
    pos_tab, seq_fa = [], []
    for at, w, head, pos, items in rows:
        sid += 2
        pos_tab.append(">spt_%d\n%s" % (sid, pos))
        if seqs is not None:
            seq_fa.append(">spt_%d%s%s\n" % (sid, head, emit_string(seqs, items)))
    if seqs is not None:
        out["supertig.pos.tab"] = "".join(pos_tab)
        out["supertig.seq.fa"] = "".join(seq_fa)
    if reads is not None:
        out["supertig.gap.data"] = "".join(gap_data)
    err.append("\nFill gaps inside scaffold sequence done\n")
    rep = [(int(lens[v // 2]), v // 2) for v in S.repeat_nodes if v % 2 == 1]
    exc_num, exc_len = len(rep), sum(r[0] for r in rep)
    LR.std_sort(rep, LR.by_len)
    rpos, rseq = [], []
    for size, c in rep:
        sid += 2
        rpos.append(">spt_%d\n\t%s\t1\t%d\t%d\tF\n" % (sid, names[c], size, size))
        if seqs is not None:
            rseq.append(">spt_%d   fragment_num:1   length:%d   lenwogap:%d   RepeatNode\n%s\n" % (sid, size, size, seqs[c]))
    out["supertig_repeat.pos.tab"] = "".join(rpos)
    if seqs is not None:
        out["supertig_repeat.seq.fa"] = "".join(rseq)
    err.append("\nTotal supertig number:          %d\nTotal supertig length[WithGap]: %d\nTotal supertig length[NoGap]:   %d\n"
               % (len(rows), tot_len, tot_len))
    err.append("\nIncluded contig number: %d  %s\n" % (inc_num, LR.fmt_float(inc_num, len(lens))))
    err.append("Included contig length: %d  %s\n" % (inc_len, LR.fmt_float(inc_len, total_len)))
    err.append("Excluded repeat contig number: %d  %s\n" % (exc_num, LR.fmt_float(exc_num, len(lens))))
    err.append("Excluded repeat contig length: %d  %s\n" % (exc_len, LR.fmt_float(exc_len, total_len)))
    err.append("\nProgram finished !\n")
    out["stderr"] = "".join(err)
    out["counters"] = dict(ctr, lowfreq=S.lowfreq, interleave=S.interleave, repeat=len(S.repeat_nodes) // 2, deleted=S.deleted,
                           scaffolds=len(rows))
    out["layout"] = [r[4] for r in rows]
    out["junctions"] = junctions
    out["repeats"] = [c for _, c in rep]
    out["stats"] = stats
    out["table"] = (first, links, ctr)
    return out


def item_len(it):
    return it[3] if it[0] == "ctg" else it[2]


def emit_string(seqs, items):
    out = []
    for it in items:
        if it[0] == "ctg":
            out.append(LR.reverse_complement(seqs[it[1]]) if it[2] else seqs[it[1]])
        else:
            out.append("N" * it[2])                # generate_Nstr, :499
    return "".join(out)


# ---- the fixtures of tests/golden/super_cases ----------------------------------------------------------------------------

def case_params(case):
    a = case["args"]
    return Params(n=int(a[a.index("-n") + 1]) if "-n" in a else DEFAULTS.n)


def load_case(D, case):
    """-> P, names, seqs, records per map file, map file names, reads (list by read index; None: in no reads file)"""
    F = LR.case_files(D, case)
    names, seqs = LR.read_contig_file(F[case["contigs"]].decode("latin-1"))
    LR.check_names(names)
    files = LR.read_lib(F[case["lib"]].decode())
    index = {}
    recs = [FR.parse_2ctg(gzip.decompress(F[f]).decode("latin-1"), len(names), index) for f in files]
    reads = [None] * len(index)
    for f in files:
        FR.load_reads(gzip.decompress(F[f + ".reads.fa.gz"]).decode("latin-1"), index, reads)
    return case_params(case), names, seqs, recs, files, reads


def run_case(D, case):
    P, names, seqs, recs, files, reads = load_case(D, case)
    res = run(P, names, [len(s) for s in seqs], recs, files, seqs, reads, prefix=case["prefix"])
    got = {"%s.%s" % (case["prefix"], k): res[k] for k in OUTPUTS}
    got["stderr.txt"] = res["stderr"]
    return got, res


def split_records(text):
    """a pos.tab or seq.fa text as a sorted list of records with their super-contig ids blanked (the tie case)"""
    recs = [r.split("\n", 1) for r in text.split(">spt_") if r]
    return sorted((h.lstrip("0123456789"), b) for h, b in recs)


def compare_outputs(case, got, want):
    """byte for byte; the case with a length tie also as a multiset of records with their ids blanked"""
    assert sorted(got) == sorted(want)
    for f in sorted(want):
        if case.get("tie") and f.endswith((".supertig.seq.fa", ".supertig.pos.tab")):
            assert split_records(got[f]) == split_records(want[f]), f
        assert got[f] == want[f], f


def golden_cases(D):
    return json.load(open(os.path.join(D, "cases.json")))
