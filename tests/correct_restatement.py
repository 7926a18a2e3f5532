"""CPU restatement of correct_error_reads (correct_error/correct.cpp correct_one_read and the per-file driver of
main_parallel_senior.cpp), written the way the HIP kernels work: a tree node is its last k-1 bases, its change
count and its (at most two) edits, so no node array or parent walk is kept.  Pinned by the correct_* goldens,
which the real reference wrote; the GPU tests compare against it on inputs no golden covers."""
import gzip

ALPHA = bytearray([4] * 256)   # bytes outside ACGTN/acgtn (and >= 128, which the reference indexes out of range)
for ch, v in ((b"A", 0), (b"a", 0), (b"N", 0), (b"n", 0), (b"C", 1), (b"c", 1), (b"G", 2), (b"g", 2), (b"T", 3), (b"t", 3)):
    ALPHA[ch[0]] = v
BASES = b"ACGT"


class Params:
    def __init__(self, k=17, m=17, c=2, x=17, n=5000000, r=75):
        self.k, self.m, self.c, self.x, self.n, self.r = k, m, c, x, n, r


def seq2bit(s):
    v = 0
    for b in s:
        v = (v << 2) | ALPHA[b]
    return v


class Table:
    """the loaded bit table (the loader's result, not the file): bit v is byte v >> 3, bit 7 - (v & 7)"""

    def __init__(self, bits, k):
        self.bits, self.total = bytes(bits), 4 ** k

    def hi(self, v):
        return v < self.total and (self.bits[v >> 3] >> (7 - (v & 7))) & 1 == 1


def _tree(read, T, P, start, end, rightward, modify, max_change, last_pos, observe=None):
    """correct_multi_bases_rightward / _leftward on a frontier of (ctx, change, edits).
    Returns (num_corrected, len_need_trim, last_pos, node_limit_hit).  observe: a list that gets one dict per tree --
    its direction and span, the sizes of the frontiers it accepted and the cumulative node count after every cycle it
    expanded (the last one is the cycle that was discarded, if any)."""
    k = P.k
    km1 = (1 << (2 * (k - 1))) - 1
    full = (1 << (2 * k)) - 1
    max_change = min(max_change, 2)
    if rightward:
        root = seq2bit(read[start - k:start - 1]) & km1
    else:
        s_bits = seq2bit(read[start:start + k - 1])
        root = 0
    front = [(root, 0, ())]
    nodes, cyc, depth, hit = 0, start, 0, 0
    step = 1 if rightward else -1
    seen = {"right": bool(rightward), "start": start, "end": end, "modify": modify, "frontiers": [], "cum": []}
    if observe is not None:
        observe.append(seen)
    while (cyc <= end) if rightward else (cyc >= end):
        here = read[cyc - 1]
        new = []
        for ctx, ch, ed in front:
            for j in range(4):
                if rightward:
                    km = ((ctx << 2) | j) & full
                    nctx = km & km1
                else:
                    km = (j << (2 * (k - 1))) | ctx | ((s_bits >> (2 * depth)) if depth < k - 1 else 0)
                    nctx = ((j << (2 * (k - 2))) | (ctx >> 2)) if k > 1 else 0
                same = BASES[j] == here
                nch = ch if same else ch + 1
                if T.hi(km) and nch <= max_change:
                    new.append((nctx, nch, ed if same else ed + ((cyc, BASES[j]),)))
        nodes += len(new)
        seen["cum"].append(nodes)
        if new and nodes < P.n:
            front = new
            seen["frontiers"].append(len(new))
        else:
            hit = int(nodes >= P.n)
            break
        cyc += step
        depth += 1
    counts = [0, 0, 0]
    for _, ch, _ in front:
        counts[ch] += 1
    mn = min(ch for _, ch, _ in front)
    trim = (end - cyc + 1) if rightward else (cyc - end + 1)
    if counts[mn] == 1 and (trim == 0 or modify):
        ed = next(e for _, ch, e in front if ch == mn)
        for pos, b in ed:
            read[pos - 1] = b
        if ed:
            if rightward and last_pos == len(read) + 1:
                last_pos = max(p for p, _ in ed)
            elif not rightward and last_pos == 0:
                last_pos = min(p for p, _ in ed)
        return mn, trim, last_pos, hit
    return 0, trim, last_pos, hit


def _runs(mask, want):
    """maximal runs of value want in mask, as (start, end) 1-based inclusive"""
    out, i, n = [], 0, len(mask)
    while i < n:
        if mask[i] != want:
            i += 1
            continue
        j = i
        while j < n and mask[j] == want:
            j += 1
        out.append((i + 1, j))
        i = j
    return out


def correct_one_read(seq, T, P, observe=None):
    """-> (corrected full-length read bytes, one_base, multi, deleted, left_trim, right_trim, node_limit_hits);
    observe: see _tree"""
    k = P.k
    read = bytearray(seq)
    L = len(read)
    nk = L - k + 1
    one = multi = accum = hits = 0
    mask = [1 if T.hi(seq2bit(read[i:i + k])) else 0 for i in range(max(nk, 0))]
    # one-base fix: low regions of exactly k k-mers between two high regions
    for s, e in _runs(mask, 0):
        if s == 1 or e == nk:
            continue
        if accum >= P.c:
            break
        if e - s + 1 != k:
            continue
        err = read[e - 1]
        for b in BASES:
            if b == err:
                continue
            read[e - 1] = b
            if all(T.hi(seq2bit(read[j:j + k])) for j in range(s - 1, e)):
                break
            read[e - 1] = err
        if read[e - 1] != err:
            one += 1
            accum += 1
            for i in range(s - 1, e):
                mask[i] = 1
    regs = [[s, e] for s, e in _runs(mask, 1) if e - s + 1 >= P.m]
    cut = int(P.m / 3)
    for r in regs:
        if r[0] != 1:
            r[0] += cut
        if r[1] != nk:
            r[1] -= cut
    if not regs:
        return bytes(read), one, multi, 1, 0, 0, hits
    fails = []
    for i in range(len(regs) - 1):
        if accum >= P.c:
            fails.extend(range(i, len(regs) - 1))
            break
        nc, tr, _, h = _tree(read, T, P, regs[i][1] + k, regs[i + 1][0] + k - 2, True, 0, P.c - accum, -1, observe)
        hits += h
        if tr == 0 and nc > 0:
            multi += nc
            accum += nc
        else:
            nc, tr, _, h = _tree(read, T, P, regs[i + 1][0] - 1, regs[i][1] + 1, False, 0, P.c - accum, -1, observe)
            hits += h
            if tr == 0 and nc > 0:
                multi += nc
                accum += nc
            else:
                fails.append(i)
    # get_max_highFreq_region
    fails.append(len(regs) - 1)
    best, cur = None, regs[0][0]
    for f in fails:
        seg = (cur, regs[f][1])
        if best is None or seg[1] - seg[0] + 1 > best[1] - best[0] + 1:
            best = seg
        if f != len(regs) - 1:
            cur = regs[f + 1][0]
    lt = rt = 0
    llast, rlast = 0, L + 1
    hs = best[0]
    if hs > 1:
        if accum < P.c:
            nc, lt, llast, h = _tree(read, T, P, hs - 1, 1, False, 1, P.c - accum, llast, observe)
            hits += h
            if nc > 0:
                multi += nc
                accum += nc
            else:
                lt, llast = hs - 1, 0
        else:
            lt, llast = hs - 1, 0
    he = best[1] + k - 1
    if he < L:
        if accum < P.c:
            nc, rt, rlast, h = _tree(read, T, P, he + 1, L, True, 1, P.c - accum, rlast, observe)
            hits += h
            if nc > 0:
                multi += nc
                accum += nc
            else:
                rt, rlast = L - he, L + 1
        else:
            rt, rlast = L - he, L + 1
    if lt > 0 or 0 < llast <= P.x:
        lt = min(lt + P.x, L)
    if rt > 0 or (rlast < L + 1 and rlast >= L - P.x + 1):
        rt = min(rt + P.x, L)
    deleted = int(L - lt - rt < P.r)
    return bytes(read), one, multi, deleted, lt, rt, hits


def read_records(path, fmt):
    """(header, sequence) pairs as parse_one_reads_file reads them: a header line must start with '@' (fq, then
    exactly 3 more lines) or '>' (fa, then 1 more line); any other line is skipped."""
    raw = gzip.open(path, "rb").read() if open(path, "rb").read(2) == b"\x1f\x8b" else open(path, "rb").read()
    lines = raw.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out, i = [], 0
    tag, extra = (b"@", 3) if fmt == 1 else (b">", 1)
    while i < len(lines):
        h = lines[i]
        i += 1
        if h[:1] == tag:
            s = lines[i] if i < len(lines) else b""
            i += extra
            out.append((b">" + h[1:] if fmt == 1 else h, s))
    return out


def _ratio(a, b):
    """(double)a / (double)b as iostream prints it: precision 6; 0 / 0 is the x86 default NaN, printed -nan"""
    if b == 0:
        return "-nan" if a == 0 else "inf"
    return "%g" % (a / b)


def record_line(head, read, one, multi, deleted, lt, rt):
    """-> (the record as the reference writes it, the kept bases)"""
    final = b"" if deleted else read[lt:len(read) - rt]
    return (b"%s\tModifiedBaseNum: %d\tFinalReadLength: %d\tLeftEndTrim: %d\tRightEndTrim: %d\tIsDeleted: %d\n%s\n"
            % (head, one + multi, len(final), lt, rt, deleted, final)), final


def correct_file(records, T, P):
    """-> (decompressed .correct.fa bytes, .correct.stat text, total node-limit hits)"""
    out = []
    raw_r = raw_b = res_r = res_b = tr_r = tr_b = del_r = one_t = multi_t = hits = 0
    for head, seq in records:
        read, one, multi, deleted, lt, rt, h = correct_one_read(seq, T, P)
        hits += h
        raw_r += 1
        raw_b += len(seq)
        line, final = record_line(head, read, one, multi, deleted, lt, rt)
        out.append(line)
        if deleted:
            del_r += 1
        else:
            one_t += one
            multi_t += multi
            if lt or rt:
                tr_r += 1
                tr_b += lt + rt
            res_r += 1
            res_b += len(final)
    allc = one_t + multi_t
    stat = ("num_raw_reads %d\nnum_raw_bases %d\nnum_result_reads %d\nnum_result_bases %d\n\nnum_trimmed_reads %d\n"
            "num_trimmed_bases %d\nnum_deleted_reads %d\n\nnum_corrected_bases_by_Fast_method %d\n"
            "num_corrected_bases_by_BBtree_method %d\nnum_corrected_bases_by_two_methods %d\n\n"
            "filter_ratio: (num_raw_bases - num_res_bases) / num_raw_bases %s\n"
            "correct_ratio: total_all_base_correct_score / num_res_bases %s\n"
            % (raw_r, raw_b, res_r, res_b, tr_r, tr_b, del_r, one_t, multi_t, allc, _ratio(raw_b - res_b, raw_b), _ratio(allc, res_b)))
    return b"".join(out), stat, hits
