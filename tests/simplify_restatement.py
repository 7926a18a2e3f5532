"""The contig stage's three simplification passes with their walks taken from traces, restated in plain Python on top of
tests/contig_restatement.py: before a pass every walk is computed on a copy of the table as the pass finds it (what the GPU
kernels do), the loops run in list order as in contig_restatement, and a trace stands for the walk if and only if
  1. the branching node is unchanged (branch rows only),
  2. the row starts at the slot and in the direction the loop has just computed,
  3. no node of the traced path, and not its last slot (unless there is none), has changed since the pass began;
otherwise the walk is made on the live table.  Changed: every node a removal deletes and every slot given to recalculate.  Counts per
pass how many walks came from a trace and how many fell back -- what bin/debruijn_contig prints under DBGK_TIMINGS -- and checks at
every use that the trace is the live walk."""
import copy

import contig_restatement as R


def snapshot(t):
    s = copy.copy(t)
    for f in ("kmer", "l_link", "r_link", "filled", "deleted", "l_num", "l_base", "r_num", "r_base", "linear"):
        setattr(s, f, list(getattr(t, f)))
    return s


class Pass:
    def __init__(self, t, o, traced=True):
        self.t, self.o, self.snap, self.changed, self.used, self.fell_back = t, o, snapshot(t) if traced else None, set(), 0, 0
        # what happened, in order, for the generator of the ordering cases (tests/golden/make_simplify_golden.py) to assert on:
        # ("walk", {...}) per walk and ("removal", {nodes, recalculated}) per removal
        self.log = []

    def branch_row(self, idx, direct, b, cutoff):
        """row 8 i + 4 side + j of the snapshot -> (start, direct, walk) or None when the row has no trace"""
        s = self.snap
        if R.depth_of(s.r_link[idx] if direct == 1 else s.l_link[idx], b) <= self.o.D:
            return None
        key, flipped = R.canonical(s, R.next_kmer(s, s.kmer[idx], b, direct))
        v = s.exist(key)
        if not s.is_linear(v):
            return None
        d1 = -direct if flipped else direct
        return v, d1

    def walk(self, row_start, branch, idx, direct, cutoff):
        """row_start: (start, direct) of the row's trace, or None; -> linear_path(idx, direct, cutoff) on the live table"""
        if self.snap is not None:
            ev = {"branch": branch, "start": idx, "direct": direct, "used": False, "traced": None,
                  "branch_changed": branch is not None and branch in self.changed, "same_start": row_start == (idx, direct)}
            self.log.append(("walk", ev))
            ok = ev["same_start"] and not ev["branch_changed"]
            if ev["same_start"]:
                p = ev["traced"] = R.linear_path(self.snap, idx, direct, cutoff)
                ev["nodes_changed"] = [v for v in p[2] if v in self.changed]
                ev["last_changed"] = p[4] != self.t.size and p[4] in self.changed
                ok = ok and not ev["nodes_changed"] and not ev["last_changed"]
            if ok:
                assert p == R.linear_path(self.t, idx, direct, cutoff), "a trace that passed the three conditions is not the live walk"
                self.used += 1
                ev["used"], ev["live"] = True, p
                return p
            self.fell_back += 1
            ev["live"] = R.linear_path(self.t, idx, direct, cutoff)
            return ev["live"]
        return R.linear_path(self.t, idx, direct, cutoff)

    def delete(self, nodes):
        self.log.append(("removal", {"nodes": list(nodes), "recalculated": []}))
        for v in nodes:
            self.t.deleted[v] = True
            self.changed.add(v)

    def recalculate(self, idx):
        if idx != self.t.size:
            self.changed.add(idx)
        self.log[-1][1]["recalculated"].append(idx)      # every recalculate follows its removal's delete
        R.recalculate(self.t, self.o, idx)


def remove_tips(t, o, tips, err, traced=True):
    ps = Pass(t, o, traced)
    rows = [(idx, -1 if ps.snap.l_num[idx] == 1 else 1) for idx in tips] if traced else [None] * len(tips)
    out, num, total = [], 0, 0
    for i, idx in enumerate(tips):
        direct = -1 if t.l_num[idx] == 1 else 1
        n, depth, nodes, s, last, mark = ps.walk(rows[i], None, idx, direct, o.I)
        avg = depth / n
        if avg <= o.P and n <= o.I:
            num += 1
            total += n
            ps.delete(nodes)
            ps.recalculate(last)
            lk, lm, rk, rm = (t.kmer[idx], "break", t.kmer_at(last), mark) if direct == 1 else (t.kmer_at(last), mark, t.kmer[idx], "break")
            out.append(">tip_%d\tlength: %d\tavgDepth: %s\tLeftEndKmer: %d %s\tRightEndKmer: %d %s\n%s\n"
                       % (num, n + t.k, R.fmt_double(avg), lk, lm, rk, rm, R.path_sequence(t, idx, direct, s)))
    err.append("\nremove total tip number:  %d\nremove total tip length:  %d\n" % (num, total))
    return "".join(out), ps


def remove_low_edges(t, o, branches, err, traced=True):
    ps = Pass(t, o, traced)
    out, num, total = [], 0, 0
    for idx in branches:
        for direct in (1, -1):
            if (t.r_num[idx] if direct == 1 else t.l_num[idx]) < 2:
                continue
            for b, d in R.branch_bases(t.r_link[idx] if direct == 1 else t.l_link[idx], o.D):
                key, flipped = R.canonical(t, R.next_kmer(t, t.kmer[idx], b, direct))
                direct1 = -direct if flipped else direct
                idx1 = t.exist(key)
                if not t.is_linear(idx1):
                    continue
                n, depth, nodes, s, last, mark = ps.walk(ps.branch_row(idx, direct, b, o.C) if traced else None, idx, idx1, direct1, o.C)
                n, depth = n + 1, depth + d
                avg = depth / n
                if n <= o.C and avg <= o.G and not t.is_linear(last):
                    num += 1
                    total += n
                    ps.delete(nodes)
                    ps.recalculate(last)
                    ps.recalculate(idx)
                    seq = R.path_sequence(t, idx1, direct1, s)
                    if direct == 1:
                        out.append(">lowedge_%d\tlength: %d\tavgDepth: %s\tLeftEndKmer: %d branch\tRightEndKmer: %d %s\n%s\n"
                                   % (num, n + t.k, R.fmt_double(avg), t.kmer[idx], t.kmer_at(last), mark, seq))
                    else:
                        out.append(">lowedge_%d    length:%d    avgDepth:%s\tLeftEndKmer: %d %s\tRightEndKmer: %d branch\n%s\n"
                                   % (num, n + t.k, R.fmt_double(avg), t.kmer_at(last), mark, t.kmer[idx], seq))
    err.append("\nremove total lowCovEdge number: %d\nremove total lowCovEdge length: %d\n" % (num, total))
    return "".join(out), ps


def remove_bubbles(t, o, branches, err, traced=True):
    ps = Pass(t, o, traced)
    out, num, total = [], 0, 0
    for idx in branches:
        if t.l_num[idx] == 2 and t.r_num[idx] == 1:
            direct, vb = -1, R.branch_bases(t.l_link[idx], o.D)
        elif t.l_num[idx] == 1 and t.r_num[idx] == 2:
            direct, vb = 1, R.branch_bases(t.r_link[idx], o.D)
        else:
            continue
        first, dirs = [], []
        for b, _ in vb[:2]:
            key, flipped = R.canonical(t, R.next_kmer(t, t.kmer[idx], b, direct))
            dirs.append(-direct if flipped else direct)
            first.append(t.exist(key))
        if not t.is_linear(first[0]) or not t.is_linear(first[1]):
            continue
        p = [ps.walk(ps.branch_row(idx, direct, vb[e][0], o.U) if traced else None, idx, first[e], dirs[e], o.U) for e in range(2)]
        avg1, avg2 = p[0][1] / p[0][0], p[1][1] / p[1][0]
        if p[0][4] != p[1][4]:
            continue
        s1, s2 = R.path_sequence(t, first[0], dirs[0], p[0][3]), R.path_sequence(t, first[1], dirs[1], p[1][3])
        if dirs[0] != dirs[1]:
            s1 = R.complement(s1[::-1])
        len1, len2 = p[0][0] + 1, p[1][0] + 1
        rate, kind = 0.0, ""
        if len1 == len2:
            rate, kind = R.count_differences(s1, s2) / len1, "SNP"
        if len1 != len2 or rate > o.E:
            s1, s2 = R.global_align(s1, s2)
            rate, kind = R.count_differences(s1, s2) / len1, "INDEL"
        if rate < o.E and abs(len1 - len2) < o.U * o.L and len1 <= o.U and len2 <= o.U:
            removed = 1 if avg1 < avg2 else 2
            ps.delete(p[removed - 1][2])
            ps.recalculate(p[removed - 1][4])
            ps.recalculate(idx)
            num += 1
            total += len1 if removed == 1 else len2
            last, mark = p[0][4], p[0][5]
            lk, lm, rk, rm = (t.kmer[idx], "branch", t.kmer_at(last), mark) if direct == 1 else (t.kmer_at(last), mark, t.kmer[idx], "branch")
            out.append(">bubble_%d\ttype: %s\tlength1: %d\tavgDepth1: %s\tlength2: %d\tavgDepth2: %s\tremoved: %d\tLeftEndKmer: %d %s\t"
                       "RightEndKmer: %d %s\n%s\n%s\n" % (num, kind, len1 + t.k, R.fmt_double(avg1), len2 + t.k, R.fmt_double(avg2), removed, lk, lm,
                                                         rk, rm, s1, s2))
    err.append("\nremove total bubble number: %d\nremove total bubble length: %d\n" % (num, total))
    return "".join(out), ps


def run_passes(t, o, traced=True, passes=None):
    """first pass and the enabled passes -> {file suffix: bytes} of the passes' files, {pass name: (requests, used, fell_back)}; the
    Pass objects go into `passes` by name where a dict is given"""
    tips, branches, _, _ = R.first_pass(t, o)
    files, counts, err = {}, {}, []
    for name, on, suffix, fn, lst, per in (("tips", o.T, "tip.fa", remove_tips, tips, 1), ("low edges", o.W, "lowedge.fa", remove_low_edges, branches, 8),
                                           ("bubbles", o.B, "bubble.fa", remove_bubbles, branches, 8)):
        if on:
            text, ps = fn(t, o, lst, err, traced)
            files[suffix] = text.encode()
            counts[name] = (per * len(lst), ps.used, ps.fell_back)
            if passes is not None:
                passes[name] = ps
    return files, counts, "".join(err)
