"""A restatement of the reference's clean_adapter and clean_lowqual (clean_illumina/) in Python, independent of the library:
what the goldens of tests/golden/clean_cases are reproduced with on the CPU and what the GPU results are compared against.

    clean_adapter.cpp:94-157    local_ungapped_aligning -> align (one pair, plain Python) and align_many (numpy, many reads)
    clean_adapter.cpp:174-231   the adapter loop, cutting, RemoveShort           -> clean_adapter
    clean_adapter.cpp:234-268   the contaminant file                              -> read_fasta
    clean_lowqual.cpp:65-188    error sum, break points, longest block            -> lowqual_block, clean_lowqual

Observers for the edge suite (tests/clean_edge_cases.py): max_cells (every cell that holds the maximum), align_lanes (the
alignment lane by lane as DESIGN.md section 7d describes the kernel, with one-token mutants), and the break points and
mutants of lowqual_block.
"""
import gzip
import json
import math
import os
import re

import numpy as np

CODE = {c: i for i, c in enumerate("ACGT")}
CODE.update({c.lower(): i for c, i in list(CODE.items())})


def reverse_complement(s):
    return "".join("TGCAN"[CODE.get(c, 4)] for c in reversed(s))


def read_fasta(text, both_strands):
    """-> [(id, sequence)] in the order the reference tries them"""
    out = []
    for rec in text.split(">")[1:]:
        head, _, body = rec.partition("\n")
        name = re.split(r"[ \t\n]+", head)[0]
        seq = body.replace("\n", "").replace(" ", "").replace("\t", "")
        out.append((name, seq))
        if both_strands == 1:
            out.append((name + " minus-strand", reverse_complement(seq)))
    return out


def parse_fastq(data):
    """bytes of a FASTQ file (already decompressed) -> [(head, read, qual)] as the reference's record loop takes them"""
    lines = data.decode("latin-1").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    recs, i = [], 0
    while i < len(lines):
        if lines[i][:1] == "@":
            got = lines[i + 1:i + 4] + ["", "", ""]
            recs.append((lines[i], got[0], got[2]))
            i += 4
        else:
            i += 1
    return recs


def load_reads(path):
    data = open(path, "rb").read()
    return parse_fastq(gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data)


NO_HIT = (-1, 0, 0, 0, 0, 0)


def align(read, ad):
    """-> (score, read_start, read_end, adapter_start, adapter_end), 1-based; score 0: no positive cell.
    Every diagonal on its own with a running sum that restarts behind a cell where it falls to <= 0; the winner over all
    diagonals is the smallest (-score, read_end, adapter_end): the first maximum of the reference's row-major scan."""
    L, A, key, best = len(read), len(ad), None, (0, 0, 0, 0, 0)
    for d in range(-(A - 1), L):
        i = max(d, 0)
        j = i - d
        s = bs = 0
        st = i
        b = None
        while i < L and j < A:
            a, c = CODE.get(read[i], 4), CODE.get(ad[j], 4)
            s += 1 if (a == c and a < 4) else -2
            if s <= 0:
                s, st = 0, i + 1
            elif s > bs:
                bs, b = s, (s, st + 1, i + 1, st + 1 - d, j + 1)
            i += 1
            j += 1
        if b and (key is None or (-b[0], b[2], b[4]) < key):
            key, best = (-b[0], b[2], b[4]), b
    return best


def align_matrix(read, ad):
    """the reference's own formulation (full matrix, strict `>` scan, walk up-left): a check of align on small inputs"""
    L, A = len(read), len(ad)
    H = [[0] * (A + 1) for _ in range(L + 1)]
    best = (0, 0, 0)
    for i in range(1, L + 1):
        for j in range(1, A + 1):
            a, c = CODE.get(read[i - 1], 4), CODE.get(ad[j - 1], 4)
            H[i][j] = max(0, H[i - 1][j - 1] + (1 if (a == c and a < 4) else -2))
            if H[i][j] > best[0]:
                best = (H[i][j], i, j)
    if not best[0]:
        return (0, 0, 0, 0, 0)
    i, j = best[1], best[2]
    while H[i][j] > 0:
        i, j = i - 1, j - 1
    return (best[0], i + 1, best[1], j + 1, best[2])


def max_cells(read, ad):
    """-> (maximum, [(read_end, adapter_end), ...] 1-based, in row-major order): every cell of the reference's matrix that holds the
    maximum; (0, []) without a positive cell.  The first one is where align_matrix ends."""
    L, A = len(read), len(ad)
    prev, top, cells = [0] * (A + 1), 0, []
    for i in range(1, L + 1):
        cur = [0] * (A + 1)
        a = CODE.get(read[i - 1], 4)
        for j in range(1, A + 1):
            cur[j] = max(0, prev[j - 1] + (1 if (a < 4 and a == CODE.get(ad[j - 1], 4)) else -2))
            if cur[j] > top:
                top, cells = cur[j], [(i, j)]
            elif cur[j] == top and top:
                cells.append((i, j))
        prev = cur
    return top, cells


ALIGN_MUTANTS = ("reset_lt", "first_ge", "fold_no_tie", "fold_re_gt", "fold_d_lt", "reduce_max_end", "reduce_min_diag", "no_128_guard",
                 "mask_5f")


def lane_code(c, mutant=None):
    """clean_code of csrc/dbgk_clean.h on a byte value: 0..3 for ACGTacgt, 4 for everything else"""
    u = c & (0x5F if mutant == "mask_5f" else 0xDF)
    letter = (mutant in ("no_128_guard", "mask_5f") or c < 128) and u in (0x41, 0x43, 0x47, 0x54)
    return ((c >> 1) ^ (c >> 2)) & 3 if letter else 4


def lane_of(read_end, adapter_end, A):
    """(lane, round) of the diagonal that holds the cell (read_end, adapter_end), both 1-based"""
    t = (read_end - adapter_end) + A - 1
    return t % 64, t // 64


def align_lanes(read, ad, mutant=None):
    """align the way DESIGN.md section 7d describes the kernel: read_len + adapter_len - 1 diagonals in rounds of 64, one diagonal
    per lane; a lane folds the best cell of each of its rounds into one with the three-key tie rule; three reductions over the 64
    lanes (maximum score, minimum read_end among those, maximum diagonal among those) name the winner.
    -> {"hit": (score, read_start, read_end, adapter_start, adapter_end), "lane", "round": of the winning diagonal,
        "ties": [(lane, round, read_end, adapter_end)] of every lane whose folded cell holds the maximum}.
    `mutant` (one of ALIGN_MUTANTS) changes one token, for tests that ask whether the crafted reads would notice."""
    L, A = len(read), len(ad)
    rc = [lane_code(ord(c), mutant) for c in read]
    ac = [(5 if v == 4 else v) for v in (lane_code(ord(c), mutant) for c in ad)]
    n_diag = L + A - 1
    lanes = [[0, 0, 0, 0, 0] for _ in range(64)]                 # bs, be, bst, bd, round of that cell
    for r0 in range(0, max(n_diag, 0), 64):
        d_lo = r0 - (A - 1)
        for lane in range(64):
            d = d_lo + lane
            s, st, rs, re_, rst = 0, max(d, 0), 0, 0, 0
            # positions outside the read hold a code that equals no adapter code: they end a run and start none
            for i in range(max(d, 0), min(L, d + A)):
                s += 1 if rc[i] == ac[i - d] else -2
                if (s < 0) if mutant == "reset_lt" else (s <= 0):
                    s, st = 0, i + 1
                elif (s >= rs) if mutant == "first_ge" else (s > rs):
                    rs, re_, rst = s, i, st
            bs, be, bst, bd, _ = lanes[lane]
            if mutant == "fold_no_tie":
                tie = False
            elif mutant == "fold_re_gt":
                tie = re_ > be or (re_ == be and d > bd)
            elif mutant == "fold_d_lt":
                tie = re_ < be or (re_ == be and d < bd)
            else:
                tie = re_ < be or (re_ == be and d > bd)
            if rs > bs or (rs == bs and rs > 0 and tie):
                lanes[lane] = [rs, re_, rst, d, r0 // 64]
    best = max(v[0] for v in lanes)
    if best <= 0:
        return {"hit": (0, 0, 0, 0, 0), "lane": None, "round": None, "ties": []}
    top = [n for n in range(64) if lanes[n][0] == best]
    end = (max if mutant == "reduce_max_end" else min)(lanes[n][1] for n in top)
    tied = [n for n in top if lanes[n][1] == end]
    diag = (min if mutant == "reduce_min_diag" else max)(lanes[n][3] for n in tied)
    src = next(n for n in tied if lanes[n][3] == diag)
    start = lanes[src][2]
    return {"hit": (best, start + 1, end + 1, start - diag + 1, end - diag + 1), "lane": src, "round": lanes[src][4],
            "ties": [(n, lanes[n][4], lanes[n][1] + 1, lanes[n][1] - lanes[n][3] + 1) for n in top]}


def first_hit(read, adapters, cutoff):
    """-> the six fields of dbgk_adapter_hit"""
    for n, (_, ad) in enumerate(adapters):
        if read and ad:
            b = align(read, ad)
            if b[0] >= cutoff:
                return (n,) + b
    return NO_HIT


_LUT = np.full(256, 4, dtype=np.uint8)
for _c, _i in CODE.items():
    _LUT[ord(_c)] = _i


def align_many(reads, adapters, cutoff, cells_per_chunk=1 << 20):
    """first_hit for many reads (bytes) at once with numpy: the matrix of the reference, one adapter column at a time over a chunk of
    reads of similar length, first row-major maximum through argmax, the walk up-left only for reads that reach the cutoff."""
    out = [NO_HIT] * len(reads)
    order = sorted(range(len(reads)), key=lambda r: len(reads[r]))
    order = [r for r in order if len(reads[r])]
    at = 0
    while at < len(order):
        Lm = len(reads[order[at]])
        n = 1
        while at + n < len(order) and (n + 1) * len(reads[order[at + n]]) <= max(cells_per_chunk, Lm):
            n += 1
            Lm = len(reads[order[at + n - 1]])
        chunk = order[at:at + n]
        at += n
        Lm = max(len(reads[r]) for r in chunk)
        codes = np.full((n, Lm), 4, dtype=np.uint8)
        for row, r in enumerate(chunk):
            codes[row, :len(reads[r])] = _LUT[np.frombuffer(reads[r], dtype=np.uint8)]
        score_of = [np.where(codes == c, 1, -2).astype(np.int16) for c in range(4)]
        none = np.full((n, Lm), -2, dtype=np.int16)
        pending = np.ones(n, dtype=bool)
        for a_idx, (_, ad) in enumerate(adapters):
            A = len(ad)
            if not A or not pending.any():
                continue
            H = np.zeros((A, n, Lm), dtype=np.int16)
            prev = np.zeros((n, Lm), dtype=np.int16)
            for j, ch in enumerate(ad):
                sc = score_of[CODE[ch]] if ch in CODE else none
                cur = H[j]
                cur[:, 0] = sc[:, 0]
                np.add(prev[:, :-1], sc[:, 1:], out=cur[:, 1:])
                np.maximum(cur, 0, out=cur)
                prev = cur
            # a positive cell behind the end of a shorter read is smaller than the cell of its diagonal it decays from: never the maximum
            flat = np.ascontiguousarray(H.transpose(1, 2, 0)).reshape(n, Lm * A)
            arg = flat.argmax(axis=1)
            top = flat[np.arange(n), arg]
            for row in np.nonzero(pending & (top >= cutoff))[0]:
                i_end, j_end = divmod(int(arg[row]), A)
                i, j = i_end, j_end
                while i >= 0 and j >= 0 and H[j, row, i] > 0:
                    i, j = i - 1, j - 1
                out[chunk[row]] = (a_idx, int(top[row]), i + 2, i_end + 1, j + 2, j_end + 1)
                pending[row] = False
    return out


def fmt_g(num, den, scale=1.0):
    """(double)num / den * scale through a default ostream; 0 / 0 prints as the reference's x86 build printed it"""
    if den == 0:
        return "-nan" if num == 0 else ("inf" if num > 0 else "-inf")
    return "%g" % (num / den * scale)


def clean_adapter(recs, adapters, cutoff=12, min_len=75, hits=None):
    """-> (text of the output file, text of the .stat file, hits)"""
    out = []
    st = dict(raw_reads=0, raw_bases=0, trim_reads=0, trim_bases=0, short_reads=0, short_bases=0, clean_reads=0, clean_bases=0)
    if hits is None:
        hits = [first_hit(s, adapters, cutoff) for _, s, _ in recs]
    for (h, s, q), hit in zip(recs, hits):
        st["raw_reads"] += 1
        st["raw_bases"] += len(s)
        a, sc, rs, re_, as_, ae = hit
        if a >= 0:
            n = len(s)
            s, q = s[:rs - 1], q[:rs - 1]
            h += "   Aligned to adapter %s,  reads_pos: %d-%d, adapter_pos: %d-%d,   score: %d" % (adapters[a][0], rs, re_, as_, ae, sc)
            st["trim_reads"] += 1
            st["trim_bases"] += n - rs + 1
        if len(s) < min_len:
            st["short_reads"] += 1
            st["short_bases"] += len(s)
            s, q, h = "", "", h + "   RemoveShort"
        else:
            st["clean_reads"] += 1
            st["clean_bases"] += len(s)
        out.append("%s\n%s\n+\n%s\n" % (h, s, q))
    stat = ("total_raw_reads:  %d\ntotal_raw_bases:  %d\n"
            "total_adapter_trimmed_reads:  %d\ntotal_adapter_trimmed_bases:  %d\t%s\n"
            "total_short_trimmed_reads:  %d\ntotal_short_trimmed_bases:  %d\t%s\n"
            "total_clean_reads:  %d\ntotal_clean_bases:  %d\t%s\n") % (
        st["raw_reads"], st["raw_bases"], st["trim_reads"], st["trim_bases"], fmt_g(st["trim_bases"], st["raw_bases"]),
        st["short_reads"], st["short_bases"], fmt_g(st["short_bases"], st["raw_bases"]),
        st["clean_reads"], st["clean_bases"], fmt_g(st["clean_bases"], st["raw_bases"]))
    return "".join(out), stat, hits


def error_table(shift):
    table = [0.0] * 256
    for i in range(100):
        if i + shift < 128:
            table[i + shift] = math.pow(10.0, -i / 10.0)
    return table


LOWQUAL_MUTANTS = ("break_ge", "longest_ge", "tail_ge", "N_keeps_quality", "n_counts_as_N", "pairwise_sum")


def _pairwise(v):
    return 0.0 if not v else (v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:]))


def lowqual_block(read, qual, cutoff, shift, table=None, breaks=None, mutant=None):
    """a record with strings of equal length -> (error_sum, start, length, trimmed): the fields of dbgk_lowqual_block.
    `breaks`, a list, receives the 0-based break points of a trimmed read; `mutant` (one of LOWQUAL_MUTANTS) changes one token."""
    table = table or error_table(shift)
    n = len(read)
    as_n = ("Nn" if mutant == "n_counts_as_N" else "N") if mutant != "N_keeps_quality" else ""
    qs = [shift if read[j] in as_n else ord(qual[j]) for j in range(n)]
    err = 0.0
    for v in qs:
        err += table[v]
    if mutant == "pairwise_sum":
        err = _pairwise([table[v] for v in qs])
    if not err > cutoff * n:
        return (err, 1 if n else 0, n, 0)
    ae, al, last, ms, ml = 0.0, 0, 0, 0, 0
    for j in range(n):
        ae += table[qs[j]]
        al += 1
        if (ae >= cutoff * al) if mutant == "break_ge" else (ae > cutoff * al):
            if breaks is not None:
                breaks.append(j)
            if (j - last >= ml) if mutant == "longest_ge" else (j - last > ml):
                ml, ms = j - last, last + 1
            ae, al, last = 0.0, 0, j + 1
    if (n - last >= ml) if mutant == "tail_ge" else (n - last > ml):
        ml, ms = n - last, last + 1
    return (err, ms, ml, 1) if 1 <= ms <= n else (err, 0, 0, 1)


def clean_lowqual(recs, cutoff=0.001, shift=33, min_len=75, blocks=None):
    """-> (text of the output file, text of the .stat file, blocks)"""
    table = error_table(shift)
    out, got = [], []
    st = dict(raw_reads=0, raw_bases=0, low_reads=0, low_bases=0, short_reads=0, short_bases=0, clean_reads=0, clean_bases=0)
    for n_rec, (h, s, q) in enumerate(recs):
        st["raw_reads"] += 1
        st["raw_bases"] += len(s)
        if len(s) != len(q):
            s = q = ""
        n = len(s)
        b = blocks[n_rec] if blocks is not None else lowqual_block(s, q, cutoff, shift, table)
        got.append(b)
        err, start, length, trimmed = b[:4]
        q = "".join(chr(shift) if c == "N" else v for c, v in zip(s, q))
        h += "    RQ: " + ("%.17g" % (err / n * 100) if n else "-nan") + "%"
        if trimmed:
            h += "  TrimLowQual"
            s, q = (s[start - 1:start - 1 + length], q[start - 1:start - 1 + length]) if start else ("", "")
            st["low_reads"] += 1
            st["low_bases"] += n - length
        if len(s) < min_len:
            st["short_reads"] += 1
            st["short_bases"] += len(s)
            h += "  FilterShort"
            s = q = ""
        if s:
            st["clean_reads"] += 1
            st["clean_bases"] += len(s)
        out.append("%s\n%s\n+\n%s\n" % (h, s, q))
    stat = "#total_raw_reads:   %d\n#total_raw_bases:   %d\n" % (st["raw_reads"], st["raw_bases"])
    for label, key in (("#filtered_lowqual", "low"), ("#filtered_short", "short"), ("#total_clean", "clean")):
        stat += "%s_reads: %d\t%s%%\n" % (label, st[key + "_reads"], fmt_g(st[key + "_reads"], st["raw_reads"], 100))
        stat += "%s_bases: %d\t%s%%\n" % (label, st[key + "_bases"], fmt_g(st[key + "_bases"], st["raw_bases"], 100))
    return "".join(out), stat, got


# ---- the golden cases (tests/golden/clean_cases/cases.json) -----------------------------------------------------------------

def case_options(case):
    """the options of a case's command line with the reference's defaults"""
    o = {"-a": None, "-b": 0, "-s": 12, "-r": 75, "-e": 0.001, "-q": 33}
    args = case["args"]
    for i in range(0, len(args), 2):
        o[args[i]] = args[i + 1] if args[i] == "-a" else (float(args[i + 1]) if args[i] == "-e" else int(args[i + 1]))
    return o


def case_adapters(cases_dir, case):
    o = case_options(case)
    return read_fasta(open(os.path.join(cases_dir, o["-a"]), encoding="latin-1").read(), o["-b"])


def run_case(cases_dir, case, hits=None, blocks=None):
    """-> {"out": text, "stat": text, "numbers": hits or blocks}"""
    o = case_options(case)
    recs = load_reads(os.path.join(cases_dir, case["input"]))
    if case["program"] == "clean_adapter":
        text, stat, nums = clean_adapter(recs, case_adapters(cases_dir, case), o["-s"], o["-r"], hits)
    else:
        text, stat, nums = clean_lowqual(recs, o["-e"], o["-q"], o["-r"], blocks)
    return {"out": text, "stat": stat, "numbers": nums}


def expected_outputs(cases_dir, case):
    d = os.path.join(cases_dir, case["name"])
    return {"out": gzip.decompress(open(os.path.join(d, "out.gz"), "rb").read()).decode("latin-1"),
            "stat": open(os.path.join(d, "out.stat"), "rb").read().decode("latin-1")}


def golden_cases(cases_dir):
    return json.load(open(os.path.join(cases_dir, "cases.json")))


NEED_ADAPTER = ("hit", "no_hit", "remove_short", "tie", "later_adapter_scores_higher")


def adapter_coverage(cases_dir, case):
    """which of the categories a clean_adapter case has to show are in it"""
    o = case_options(case)
    adapters = case_adapters(cases_dir, case)
    seen = set()
    for _, s, _ in load_reads(os.path.join(cases_dir, case["input"])):
        hit = first_hit(s, adapters, o["-s"])
        seen.add("hit" if hit[0] >= 0 else "no_hit")
        kept = hit[2] - 1 if hit[0] >= 0 else len(s)
        if kept < o["-r"]:
            seen.add("remove_short")
        if hit[0] >= 0:
            ad = adapters[hit[0]][1]
            if _count_max_cells(s, ad) > 1:
                seen.add("tie")
            if any(align(s, later)[0] > hit[1] for _, later in adapters[hit[0] + 1:] if later):
                seen.add("later_adapter_scores_higher")
    return seen


def _count_max_cells(read, ad):
    L, A = len(read), len(ad)
    prev, top, count = [0] * (A + 1), 0, 0
    for i in range(1, L + 1):
        cur = [0] * (A + 1)
        for j in range(1, A + 1):
            a, c = CODE.get(read[i - 1], 4), CODE.get(ad[j - 1], 4)
            cur[j] = max(0, prev[j - 1] + (1 if (a == c and a < 4) else -2))
            if cur[j] > top:
                top, count = cur[j], 1
            elif cur[j] == top and top:
                count += 1
        prev = cur
    return count
