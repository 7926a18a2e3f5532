"""The bubbles pass of the contig stage with its alignments computed when the pass begins, restated in plain Python on top of
tests/simplify_restatement.py (the traced walks) and tests/contig_restatement.py (global_align).

When the pass begins, every entry of its list that is a bubble in the pass's traces is a CANDIDATE: two edges on one side and one
on the other, both arm rows traced, both arms ending on the same node.  Its two strings are composed from the traces as
remove_bubbles composes them, and the candidates that remove_bubbles would align -- unequal lengths, or equal lengths and a
difference rate above -E -- are SUBMITTED (none with host=True, the hook align_host; with stale=True, the hook align_stale, each
with its two strings exchanged, so that no result is ever the one the loop asks for).  A submitted pair with a string longer than
max_len is TOO LONG and has no result.  In the ordered loop a result is USED if and only if
  1. this list entry submitted a pair,
  2. the two strings the loop holds at that moment are equal to the submitted ones,
  3. the pair is not too long;
every other alignment of the pass is made ON THE HOST.  These are the five counts bin/debruijn_contig prints under DBGK_TIMINGS as
`Contig stage aligned arms (bubbles): candidates C submitted S too long T used U aligned on the host H ...`.  The walks go through
the three-condition rule of simplify_restatement, so the pass's trace counts come out as there."""
import contig_restatement as R
import simplify_restatement as S

MAX_LEN = 256   # DBGK_ALIGN_MAX_LEN


def arms(t, o, idx):
    """the bubble test at the head of remove_bubbles' loop -> (direct, the two branch bases) or None"""
    if t.l_num[idx] == 2 and t.r_num[idx] == 1:
        direct, vb = -1, R.branch_bases(t.l_link[idx], o.D)
    elif t.l_num[idx] == 1 and t.r_num[idx] == 2:
        direct, vb = 1, R.branch_bases(t.r_link[idx], o.D)
    else:
        return None
    return (direct, [b for b, _ in vb[:2]]) if len(vb) >= 2 else None


def compose(t, first, dirs, steps):
    s1, s2 = R.path_sequence(t, first[0], dirs[0], steps[0]), R.path_sequence(t, first[1], dirs[1], steps[1])
    if dirs[0] != dirs[1]:
        s1 = R.complement(s1[::-1])
    return s1, s2


def needs_aligning(o, s1, s2, len1, len2):
    return len1 != len2 or R.count_differences(s1, s2) / len1 > o.E


def collect(ps, o, branches, host=False, every=None, stale=False):
    """-> candidates, {entry index: (s1, s2)} of the submitted pairs, from the snapshot of the pass; every candidate's
    (entry index, s1, s2, len1, len2) is appended to `every` where a list is given"""
    snap, candidates, submitted = ps.snap, 0, {}
    for i, idx in enumerate(branches):
        a = arms(snap, o, idx)
        if a is None:
            continue
        direct, vb = a
        rows = [ps.branch_row(idx, direct, b, o.U) for b in vb]
        if rows[0] is None or rows[1] is None:
            continue
        p = [R.linear_path(snap, v, d, o.U) for v, d in rows]
        if p[0][4] != p[1][4]:
            continue
        candidates += 1
        s1, s2 = compose(snap, [r[0] for r in rows], [r[1] for r in rows], [p[0][3], p[1][3]])
        if every is not None:
            every.append((i, s1, s2, p[0][0] + 1, p[1][0] + 1))
        if not host and needs_aligning(o, s1, s2, p[0][0] + 1, p[1][0] + 1):
            submitted[i] = (s2, s1) if stale else (s1, s2)
    return candidates, submitted


def remove_bubbles(t, o, branches, err, traced=True, host=False, max_len=MAX_LEN, stale=False):
    """simplify_restatement.remove_bubbles with the rule above -> text of bubble.fa, the Pass, the five counts (None without traces:
    the program prints no such line when it did not trace) and the log of alignments [(entry, used, len1, len2, submitted)]"""
    ps = S.Pass(t, o, traced)
    candidates, submitted = collect(ps, o, branches, host, stale=stale) if traced else (0, {})
    too_long = {i for i, (a, b) in submitted.items() if len(a) > max_len or len(b) > max_len}
    used = on_host = 0
    log = []
    out, num, total = [], 0, 0
    for i, idx in enumerate(branches):
        a = arms(t, o, idx)
        if a is None:
            continue
        direct, vb = a
        first, dirs = [], []
        for b in vb:
            key, flipped = R.canonical(t, R.next_kmer(t, t.kmer[idx], b, direct))
            dirs.append(-direct if flipped else direct)
            first.append(t.exist(key))
        if not t.is_linear(first[0]) or not t.is_linear(first[1]):
            continue
        p = [ps.walk(ps.branch_row(idx, direct, vb[e], o.U) if traced else None, idx, first[e], dirs[e], o.U) for e in range(2)]
        avg1, avg2 = p[0][1] / p[0][0], p[1][1] / p[1][0]
        if p[0][4] != p[1][4]:
            continue
        s1, s2 = compose(t, first, dirs, [p[0][3], p[1][3]])
        len1, len2 = p[0][0] + 1, p[1][0] + 1
        rate, kind = 0.0, ""
        if len1 == len2:
            rate, kind = R.count_differences(s1, s2) / len1, "SNP"
        if len1 != len2 or rate > o.E:
            from_device = i in submitted and submitted[i] == (s1, s2) and i not in too_long
            used += from_device
            on_host += not from_device
            log.append((i, from_device, len1, len2, i in submitted))
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
    counts = dict(candidates=candidates, submitted=len(submitted), too_long=len(too_long), used=used, host=on_host)
    return "".join(out), ps, counts, log


def run_passes(t, o, traced=True, host=False, max_len=MAX_LEN, stale=False):
    """first pass, tips, low edges (simplify_restatement) and the bubbles pass above -> dict: files {suffix: bytes} of the passes'
    files, counts {pass: (requests, used, fell back)}, aligned (the five alignment counts; None when the bubbles pass is off), log (one
    entry per alignment of the pass), pairs {entry index: (s1, s2)} as submitted, every (all candidates with their strings)"""
    tips, branches, _, _ = R.first_pass(t, o)
    files, counts, err = {}, {}, []
    for name, on, suffix, fn, lst, per in (("tips", o.T, "tip.fa", S.remove_tips, tips, 1), ("low edges", o.W, "lowedge.fa", S.remove_low_edges, branches, 8)):
        if on:
            text, ps = fn(t, o, lst, err, traced)
            files[suffix] = text.encode()
            counts[name] = (per * len(lst), ps.used, ps.fell_back)
    aligned, log, pairs, every = None, [], {}, []
    if o.B:
        if traced:
            pairs = collect(S.Pass(t, o, True), o, branches, host, every, stale)[1]
        text, ps, aligned, log = remove_bubbles(t, o, branches, err, traced, host, max_len, stale)
        files["bubble.fa"] = text.encode()
        counts["bubbles"] = (8 * len(branches), ps.used, ps.fell_back)
    return dict(files=files, counts=counts, aligned=aligned, log=log, pairs=pairs, every=every, stderr="".join(err))
