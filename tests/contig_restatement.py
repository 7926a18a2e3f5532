"""Line-by-line restatement of the contig stage (DBG_contig/contig.cpp, global_aligning.cpp) on a host-layout table: the first pass,
the three simplification passes, the serial read-out, the sort of the reference's C++ library, the seven files and the stderr
counters.  Plain Python, no GPU; what the host stage and the kernels are compared with.  Line numbers name contig.cpp."""
import numpy as np

M64 = (1 << 64) - 1
BASES, C_BASES = "ACGT", "TGCA"
MARK = ("break", "branch")
REPEAT = ("Unknown", "Unique", "Repeat")


def hash_code(h):   # kmerSet.h:105-116
    h = (h + (~(h << 32) & M64)) & M64
    h ^= h >> 22
    h = (h + (~(h << 13) & M64)) & M64
    h ^= h >> 8
    h = (h + (h << 3)) & M64
    h ^= h >> 15
    h = (h + (~(h << 27) & M64)) & M64
    h ^= h >> 31
    return h


def revcomp(kbit, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (kbit & 3))
        kbit >>= 2
    return r


def bit2seq(kbit, k):
    return "".join(BASES[(kbit >> (2 * (k - 1 - j))) & 3] for j in range(k))


def fmt_double(x):
    """ostream << double: six significant digits, %g"""
    return "%g" % x


SUFFIXES = ["kmer.freq", "tip.fa", "lowedge.fa", "bubble.fa", "seq.fa", "seq.depth", "small.fa", "small.depth"]


def load_case(path):
    """one golden case, a compressed .npz written by tests/golden/make_contig_golden.py -> dict: args, k, reads (the one-line FASTA
    file as bytes), stderr, shows, files {suffix: bytes}, and the table arrays"""
    import json
    z = np.load(path)
    c = {"args": json.loads(z["args"].tobytes()), "shows": json.loads(z["shows"].tobytes()), "stderr": z["stderr"].tobytes().decode("latin-1"),
         "reads": z["reads"].tobytes(), "files": {s: z["out." + s].tobytes() for s in SUFFIXES if "out." + s in z.files}}
    c["k"] = int(c["args"][c["args"].index("-k") + 1])
    for f in ("table_size", "slots", "kmers", "l_links", "r_links"):
        c[f] = z[f]
    return c


class Table:
    """size slots; occupied slot i holds kmer[i], l_link[i], r_link[i]; filled[i] / deleted[i] are the two flag bits"""

    def __init__(self, size, k):
        self.size, self.k = size, k
        self.kmer = [0] * size
        self.l_link = [0] * size
        self.r_link = [0] * size
        self.filled = [False] * size
        self.deleted = [False] * size
        # link records (contig.h:31-42)
        self.l_num = [0] * size
        self.l_base = [0] * size
        self.r_num = [0] * size
        self.r_base = [0] * size
        self.linear = [False] * size
        self.kept = {"deep_tips": 0, "diverged_bubbles": 0}   # candidates the passes looked at and left in place

    @classmethod
    def from_case(cls, case):
        """a golden case (load_case below): the occupied slots of the reference's table"""
        t = cls(int(case["table_size"]), case["k"])
        for i, kmer, l, r in zip(case["slots"].tolist(), case["kmers"].tolist(), case["l_links"].tolist(), case["r_links"].tolist()):
            t.kmer[i], t.l_link[i], t.r_link[i], t.filled[i] = kmer, l, r, True
        return t

    @classmethod
    def from_image(cls, raw, k):
        """the raw image DBGK_DUMP_TABLE writes: size, count, the node array, the nul_flag bytes"""
        size = int(np.frombuffer(raw, "<u8", 1)[0])
        nodes = np.frombuffer(raw, np.dtype([("kmer", "<u8"), ("l", "<u4"), ("r", "<u4")]), size, 16)
        nul = np.frombuffer(raw, np.uint8, size // 8 + 1, 16 + 16 * size)
        t = cls(size, k)
        for i in np.nonzero(np.unpackbits(nul)[:size])[0]:
            i = int(i)
            t.kmer[i], t.l_link[i], t.r_link[i], t.filled[i] = int(nodes["kmer"][i]), int(nodes["l"][i]), int(nodes["r"][i]), True
        return t

    def insert(self, kmer, l_link, r_link):
        """add_node_to_kmerset (kmerSet.cpp:253-273) -> slot"""
        s = hash_code(kmer) % self.size
        while self.filled[s]:
            s = 0 if s + 1 == self.size else s + 1
        self.kmer[s], self.l_link[s], self.r_link[s], self.filled[s] = kmer, l_link, r_link, True
        return s

    def exist(self, kmer):   # exist_kmerset, kmerSet.cpp:280-302
        s = hash_code(kmer) % self.size
        for _ in range(self.size):
            if not self.filled[s]:
                return self.size
            if self.kmer[s] == kmer:
                return self.size if self.deleted[s] else s
            s = 0 if s + 1 == self.size else s + 1
        return self.size

    def is_linear(self, i):
        return i != self.size and self.linear[i]

    def kmer_at(self, i):   # array[size].kmer reads the word behind the table: 0
        return 0 if i == self.size else self.kmer[i]

    # arrays as capi.ContigBuilder.set_table takes them
    def arrays(self):
        from dbg_assembly_amd import capi
        a = np.zeros(self.size, dtype=capi.NODE_DTYPE)
        a["kmer"], a["l_link"], a["r_link"] = self.kmer, self.l_link, self.r_link
        nul = np.packbits(np.array(self.filled + [False] * 8, dtype=np.uint8))[:self.size // 8 + 1]
        dele = np.packbits(np.array(self.deleted + [False] * 8, dtype=np.uint8))[:self.size // 8 + 1]
        kl = np.array([self.l_num[i] | self.l_base[i] << 2 | self.r_num[i] << 4 | self.r_base[i] << 6 | (0x100 if self.linear[i] else 0)
                       for i in range(self.size)], dtype=np.uint16)
        return a, nul, dele, kl


def depth_of(link, base):   # get_next_kmer_depth, kmerSet.cpp:341-344
    return (link >> ((3 - base) * 8)) & 0xff


def next_kmer(t, kmer, base, direct):   # contig.h:119-130
    if direct == 1:
        return ((kmer << 2) | base) & ((1 << (2 * t.k)) - 1)
    return (kmer >> 2) + (base << ((t.k - 1) * 2))


def canonical(t, kmer):
    rc = revcomp(kmer, t.k)
    return (kmer, False) if kmer < rc else (rc, True)


class Options:
    def __init__(self, D=2, T=1, I=100, P=3.0, W=1, C=100, G=3.0, B=1, U=100, L=0.1, E=0.1, M=125):
        self.D, self.T, self.I, self.P, self.W, self.C, self.G, self.B, self.U, self.L, self.E, self.M = D, T, I, P, W, C, G, B, U, L, E, M

    @classmethod
    def from_args(cls, args):
        """the option list of a golden case: ["-k", "31", "-D", "2", ...]"""
        o, kinds = cls(), {"D": int, "T": int, "I": int, "P": float, "W": int, "C": int, "G": float, "B": int, "U": int, "L": float,
                           "E": float, "M": int}
        for a, v in zip(args[::2], args[1::2]):
            if a[1:] in kinds:
                setattr(o, a[1:], kinds[a[1:]](v))
        return o


def side_links(link, cutoff):
    num, base, best = 0, 0, 0
    for j in range(4):
        d = depth_of(link, j)
        if d > cutoff:
            num = min(num + 1, 3)
            if best < d:
                best, base = d, j
    return num, base


def first_pass(t, o):
    """calculate_kmer_links, :107-205 -> tips, branches, DepthStat, (total, deleted, linear)"""
    tips, branches, stat = [], [], [0] * 256
    total = deleted = linear = 0
    for i in range(t.size):
        if not t.filled[i]:
            continue
        for link in (t.l_link[i], t.r_link[i]):
            for j in range(4):
                stat[depth_of(link, j)] += 1
        t.l_num[i], t.l_base[i] = side_links(t.l_link[i], o.D)
        t.r_num[i], t.r_base[i] = side_links(t.r_link[i], o.D)
        total += 1
        if t.l_num[i] == 0 and t.r_num[i] == 0:
            t.deleted[i] = True
            deleted += 1
        if t.l_num[i] == 1 and t.r_num[i] == 1:
            t.linear[i] = True
            linear += 1
        if t.l_num[i] + t.r_num[i] == 1:
            tips.append(i)
        if t.l_num[i] > 1 or t.r_num[i] > 1:
            branches.append(i)
    return tips, branches, stat, (total, deleted, linear)


def recalculate(t, o, idx):   # :210-277
    if idx == t.size:
        return
    res = []
    for direct, link in ((-1, t.l_link[idx]), (1, t.r_link[idx])):
        num, base, best = 0, 0, 0
        for j in range(4):
            d = depth_of(link, j)
            if d > o.D:
                key, _ = canonical(t, next_kmer(t, t.kmer[idx], j, direct))
                if t.exist(key) != t.size:
                    num = min(num + 1, 3)
                    if best < d:
                        best, base = d, j
                else:
                    link &= ~(0xff << ((3 - j) * 8)) & 0xffffffff
        res.append((num, base, link))
    (t.l_num[idx], t.l_base[idx], t.l_link[idx]), (t.r_num[idx], t.r_base[idx], t.r_link[idx]) = res
    t.linear[idx] = t.l_num[idx] == 1 and t.r_num[idx] == 1


def linear_path(t, idx, direct, len_cutoff):
    """get_linear_path, :779-827 -> len, depth, nodes, str, last, mark"""
    original, n, depth, nodes, s = direct, 0, 0, [], []
    while True:
        n += 1
        nodes.append(idx)
        if direct == 1:
            b = t.r_base[idx]
            depth += depth_of(t.r_link[idx], b)
            s.append(BASES[b] if original == 1 else C_BASES[b])
        else:
            b = t.l_base[idx]
            depth += depth_of(t.l_link[idx], b)
            s.append(C_BASES[b] if original == 1 else BASES[b])
        key, flipped = canonical(t, next_kmer(t, t.kmer[idx], b, direct))
        if flipped:
            direct = -direct
        idx = t.exist(key)
        if not t.is_linear(idx) or n >= len_cutoff:
            if idx == t.size:
                mark = "break"
            else:
                mark = "break" if t.l_num[idx] == 0 or t.r_num[idx] == 0 else "branch"
            return n, depth, nodes, "".join(s), idx, mark


def path_sequence(t, first, direct, steps):
    kmer = bit2seq(t.kmer[first], t.k)
    return kmer + steps if direct == 1 else steps[::-1] + kmer


def remove_tips(t, o, tips, err):   # :281-355
    out, num, total = [], 0, 0
    for idx in tips:
        direct = -1 if t.l_num[idx] == 1 else 1
        n, depth, nodes, s, last, mark = linear_path(t, idx, direct, o.I)
        avg = depth / n
        t.kept["deep_tips"] += 1 if avg > o.P and n < o.I else 0   # (a walk stops at -I steps, so length alone keeps no tip: :308, :810)
        if avg <= o.P and n <= o.I:
            num += 1
            total += n
            for v in nodes:
                t.deleted[v] = True
            recalculate(t, o, last)
            lk, lm, rk, rm = (t.kmer[idx], "break", t.kmer_at(last), mark) if direct == 1 else (t.kmer_at(last), mark, t.kmer[idx], "break")
            out.append(">tip_%d\tlength: %d\tavgDepth: %s\tLeftEndKmer: %d %s\tRightEndKmer: %d %s\n%s\n"
                       % (num, n + t.k, fmt_double(avg), lk, lm, rk, rm, path_sequence(t, idx, direct, s)))
    err.append("\nremove total tip number:  %d\nremove total tip length:  %d\n" % (num, total))
    return "".join(out)


def branch_bases(link, cutoff):   # :361-370
    return [(j, depth_of(link, j)) for j in range(4) if depth_of(link, j) > cutoff]


def remove_low_edges(t, o, branches, err):   # :601-776
    out, num, total = [], 0, 0
    for idx in branches:
        for direct in (1, -1):
            if (t.r_num[idx] if direct == 1 else t.l_num[idx]) < 2:
                continue
            for b, d in branch_bases(t.r_link[idx] if direct == 1 else t.l_link[idx], o.D):
                key, flipped = canonical(t, next_kmer(t, t.kmer[idx], b, direct))
                direct1 = -direct if flipped else direct
                idx1 = t.exist(key)
                if not t.is_linear(idx1):
                    continue
                n, depth, nodes, s, last, mark = linear_path(t, idx1, direct1, o.C)
                n, depth = n + 1, depth + d
                avg = depth / n
                if n <= o.C and avg <= o.G and not t.is_linear(last):
                    num += 1
                    total += n
                    for v in nodes:
                        t.deleted[v] = True
                    recalculate(t, o, last)
                    recalculate(t, o, idx)
                    seq = path_sequence(t, idx1, direct1, s)
                    if direct == 1:
                        out.append(">lowedge_%d\tlength: %d\tavgDepth: %s\tLeftEndKmer: %d branch\tRightEndKmer: %d %s\n%s\n"
                                   % (num, n + t.k, fmt_double(avg), t.kmer[idx], t.kmer_at(last), mark, seq))
                    else:
                        out.append(">lowedge_%d    length:%d    avgDepth:%s\tLeftEndKmer: %d %s\tRightEndKmer: %d branch\n%s\n"
                                   % (num, n + t.k, fmt_double(avg), t.kmer_at(last), mark, t.kmer[idx], seq))
    err.append("\nremove total lowCovEdge number: %d\nremove total lowCovEdge length: %d\n" % (num, total))
    return "".join(out)


def count_differences(a, b):   # :587-595
    return sum(1 for x, y in zip(a, b) if x != y and x != "-" and y != "-")


def global_align(si, sj):   # global_aligning.cpp:98-182
    gap, ni, nj = -5, len(si), len(sj)
    w = nj + 1
    score, frm = [0] * ((ni + 1) * w), [0] * ((ni + 1) * w)
    for j in range(1, nj + 1):
        score[j], frm[j] = gap * j, 1
    for i in range(1, ni + 1):
        score[i * w], frm[i * w] = gap * i, 2
    for i in range(1, ni + 1):
        for j in range(1, nj + 1):
            sub = score[(i - 1) * w + j - 1] + (3 if si[i - 1] == sj[j - 1] else -5)
            gi, gj = score[i * w + j - 1] + gap, score[(i - 1) * w + j] + gap
            if sub >= gi and sub >= gj:
                best, d = sub, 0
            elif gi > sub and gi >= gj:
                best, d = gi, 1
            else:
                best, d = gj, 2
            score[i * w + j], frm[i * w + j] = best, d
    ai, aj, i, j = [], [], ni, nj
    while True:
        d = frm[i * w + j]
        if d == 0:
            i, j = i - 1, j - 1
            ai.append(si[i]), aj.append(sj[j])
        elif d == 1:
            j -= 1
            ai.append("-"), aj.append(sj[j])
        else:
            i -= 1
            ai.append(si[i]), aj.append("-")
        if not (i > 0 or j > 0):
            break
    return "".join(ai[::-1]), "".join(aj[::-1])


def complement(s):
    return "".join(C_BASES[BASES.index(c)] for c in s)


def remove_bubbles(t, o, branches, err):   # :375-582
    out, num, total = [], 0, 0
    for idx in branches:
        if t.l_num[idx] == 2 and t.r_num[idx] == 1:
            direct, vb = -1, branch_bases(t.l_link[idx], o.D)
        elif t.l_num[idx] == 1 and t.r_num[idx] == 2:
            direct, vb = 1, branch_bases(t.r_link[idx], o.D)
        else:
            continue
        first, dirs = [], []
        for b, _ in vb[:2]:
            key, flipped = canonical(t, next_kmer(t, t.kmer[idx], b, direct))
            dirs.append(-direct if flipped else direct)
            first.append(t.exist(key))
        if not t.is_linear(first[0]) or not t.is_linear(first[1]):
            continue
        p = [linear_path(t, first[e], dirs[e], o.U) for e in range(2)]
        avg1, avg2 = p[0][1] / p[0][0], p[1][1] / p[1][0]
        if p[0][4] != p[1][4]:
            continue
        s1, s2 = path_sequence(t, first[0], dirs[0], p[0][3]), path_sequence(t, first[1], dirs[1], p[1][3])
        if dirs[0] != dirs[1]:
            s1 = complement(s1[::-1])
        len1, len2 = p[0][0] + 1, p[1][0] + 1
        rate, kind = 0.0, ""
        if len1 == len2:
            rate, kind = count_differences(s1, s2) / len1, "SNP"
        if len1 != len2 or rate > o.E:
            s1, s2 = global_align(s1, s2)
            rate, kind = count_differences(s1, s2) / len1, "INDEL"
        t.kept["diverged_bubbles"] += 1 if rate >= o.E and len1 <= o.U and len2 <= o.U else 0
        if rate < o.E and abs(len1 - len2) < o.U * o.L and len1 <= o.U and len2 <= o.U:
            removed = 1 if avg1 < avg2 else 2
            for v in p[removed - 1][2]:
                t.deleted[v] = True
            recalculate(t, o, p[removed - 1][4])
            recalculate(t, o, idx)
            num += 1
            total += len1 if removed == 1 else len2
            last, mark = p[0][4], p[0][5]
            lk, lm, rk, rm = (t.kmer[idx], "branch", t.kmer_at(last), mark) if direct == 1 else (t.kmer_at(last), mark, t.kmer[idx], "branch")
            out.append(">bubble_%d\ttype: %s\tlength1: %d\tavgDepth1: %s\tlength2: %d\tavgDepth2: %s\tremoved: %d\tLeftEndKmer: %d %s\t"
                       "RightEndKmer: %d %s\n%s\n%s\n" % (num, kind, len1 + t.k, fmt_double(avg1), len2 + t.k, fmt_double(avg2), removed, lk, lm,
                                                         rk, rm, s1, s2))
    err.append("\nremove total bubble number: %d\nremove total bubble length: %d\n" % (num, total))
    return "".join(out)


def linear_seq(t, deleted, idx, direct):
    """get_linear_seq, :832-896 -> len, depth, bases, depth bytes, last, mark (0/1), repeat (0/1/2)"""
    original, n, depth, s, ds = direct, 0, 0, [], []
    while True:
        n += 1
        if direct == 1:
            b = t.r_base[idx]
            d = depth_of(t.r_link[idx], b)
            s.append(BASES[b] if original == 1 else C_BASES[b])
        else:
            b = t.l_base[idx]
            d = depth_of(t.l_link[idx], b)
            s.append(C_BASES[b] if original == 1 else BASES[b])
        depth += d
        ds.append(d - 1 if d in (10, 62) else d)
        key, flipped = canonical(t, next_kmer(t, t.kmer[idx], b, direct))
        if flipped:
            direct = -direct
        idx = exist_with(t, deleted, key)
        if idx == t.size:
            return n, depth, "".join(s), ds, idx, 0, 0
        if not t.linear[idx]:
            if t.l_num[idx] == 0 or t.r_num[idx] == 0:
                return n, depth, "".join(s), ds, idx, 0, 0
            rep = 2 if (direct == 1 and t.r_num[idx] > 1) or (direct == -1 and t.l_num[idx] > 1) else 1
            return n, depth, "".join(s), ds, idx, 1, rep
        deleted[idx] = True


def exist_with(t, deleted, kmer):
    s = hash_code(kmer) % t.size
    for _ in range(t.size):
        if not t.filled[s]:
            return t.size
        if t.kmer[s] == kmer:
            return t.size if deleted[s] else s
        s = 0 if s + 1 == t.size else s + 1
    return t.size


def read_out_contigs(t):
    """read_out_contig's scan, :930-1011 -> per contig in scan order a dict (record fields, bases, depths); t is left as it is"""
    deleted, out = list(t.deleted), []
    for i in range(t.size):
        if not t.filled[i] or deleted[i] or not t.linear[i]:
            continue
        rn, rd, rs, rds, rlast, rmark, rrep = linear_seq(t, deleted, i, 1)
        ln, ld, ls, lds, llast, lmark, lrep = linear_seq(t, deleted, i, -1)
        deleted[i] = True
        avg = (ld + rd) / (ln + rn)
        md = int(avg) & 0xff
        if md in (10, 62):
            md -= 1
        out.append(dict(anchor=i, left_end=llast, right_end=rlast, left_len=ln, right_len=rn, left_depth=ld, right_depth=rd, left_mark=lmark,
                        right_mark=rmark, left_repeat=lrep, right_repeat=rrep, mid_depth=md, avg=avg,
                        bases=ls[::-1] + bit2seq(t.kmer[i], t.k) + rs, depths=bytes(lds[::-1] + [md] * t.k + rds)))
    return out


def order_dependent_nodes(t):
    """the live linear nodes whose chain the kernels hand to the host walker: a step that the neighbour's link back does not answer,
    a step of a node onto itself, a cycle -- and every node chained to such a node by answered steps"""
    live = [i for i in range(t.size) if t.filled[i] and not t.deleted[i] and t.linear[i]]
    succ = {}
    for u in live:
        for d in (1, -1):
            b = t.r_base[u] if d == 1 else t.l_base[u]
            key, flipped = canonical(t, next_kmer(t, t.kmer[u], b, d))
            v = t.exist(key)
            succ[(u, d)] = (v, -d if flipped else d) if t.is_linear(v) else None
    marked, nbr = set(), {}
    for (u, d), nx in succ.items():
        if nx is None:
            continue
        v, d2 = nx
        if succ.get((v, -d2)) != (u, -d) or v == u:
            marked.update((u, v))
        else:
            nbr.setdefault(u, []).append(v)
    seen, bad = set(), set()
    for u in live:
        if u in seen:
            continue
        comp, stack = [], [u]
        seen.add(u)
        while stack:
            x = stack.pop()
            comp.append(x)
            for y in nbr.get(x, []):
                if y not in seen:
                    seen.add(y)
                    stack.append(y)
        ends = sum(1 for x in comp if len(nbr.get(x, [])) < 2)
        if ends == 0 or any(x in marked for x in comp):   # a cycle has no node with a free side
            bad.update(comp)
    return bad


def std_sort(a, less):
    """std::sort of libstdc++ (bits/stl_algo.h: introsort, threshold 16, median of three to the front, final insertion sort):
    equal keys end where its swaps leave them"""
    def insertion(lo, hi, guarded):
        for i in range(lo + (1 if guarded else 0), hi):
            v = a[i]
            if guarded and less(v, a[lo]):
                a[lo + 1:i + 1] = a[lo:i]
                a[lo] = v
            else:
                j = i
                while less(v, a[j - 1]):
                    a[j] = a[j - 1]
                    j -= 1
                a[j] = v

    def loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                raise NotImplementedError("std::sort fell back to heap sort: not restated")
            depth -= 1
            mid = first + (last - first) // 2
            x, y, z = first + 1, mid, last - 1
            if less(a[x], a[y]):
                m = y if less(a[y], a[z]) else z if less(a[x], a[z]) else x
            else:
                m = x if less(a[x], a[z]) else z if less(a[y], a[z]) else y
            a[first], a[m] = a[m], a[first]
            lo, hi = first + 1, last
            while True:
                while less(a[lo], a[first]):
                    lo += 1
                hi -= 1
                while less(a[first], a[hi]):
                    hi -= 1
                if not lo < hi:
                    break
                a[lo], a[hi] = a[hi], a[lo]
                lo += 1
            loop(lo, last, depth)
            last = lo

    n = len(a)
    if n:
        loop(0, n, 2 * (n.bit_length() - 1))
        if n > 16:
            insertion(0, 16, True)
            insertion(16, n, False)
        else:
            insertion(0, n, True)
    return a


def contig_files(t, o, contigs, err):
    """:1003-1043 -> seq.fa, seq.depth, small.fa, small.depth as bytes"""
    items, brk, brn = [], 0, 0
    for c in contigs:
        n = c["left_len"] + t.k + c["right_len"]
        for m in (c["right_mark"], c["left_mark"]):
            if m:
                brn += 1
            else:
                brk += 1
        head = "\tlength: %d\tavgDepth: %s\tLeftEndKmer: %d %s-%s\tRightEndKmer: %d %s-%s\t%s\n%s\n" % (
            n, "%.17g" % c["avg"], t.kmer_at(c["left_end"]), MARK[c["left_mark"]], REPEAT[c["left_repeat"]], t.kmer_at(c["right_end"]),
            MARK[c["right_mark"]], REPEAT[c["right_repeat"]], "RepeatNode" if c["left_repeat"] == 2 and c["right_repeat"] == 2 else "", c["bases"])
        items.append((len(c["bases"]), head.encode(), c["depths"]))
    std_sort(items, lambda x, y: y[0] < x[0])
    files, stats, cid = [[], [], [], []], [0, 0, 0, 0], 1
    for n, head, depths in items:
        w = 0 if n >= o.M else 2
        files[w].append(b">ctg_%d" % cid + head)
        files[w + 1].append(b">ctg_%d\n" % cid + depths + b"\n")
        stats[w] += 1
        stats[w + 1] += n
        cid += 2
    err.append("\ncontig break-point number:     %d\ncontig branch-point number:    %d\n" % (brk, brn))
    err.append("\nTotal contig number:   %d\nTotal contig length:   %d\n" % (stats[0], stats[1]))
    err.append("\nTotal small edge number:   %d\nTotal small edge length:   %d\n" % (stats[2], stats[3]))
    return [b"".join(f) for f in files]


def run_stage(t, o):
    """build_contig_sequence, :54-102 -> {file suffix: bytes}, the stderr counter lines (str), the contigs in scan order"""
    err = []
    tips, branches, stat, (total, deleted, linear) = first_pass(t, o)
    files = {"kmer.freq": ("Kmer_depth\tAppear_times\n" + "".join("%d\t%d\n" % (i, stat[i]) for i in range(1, 256))).encode()}
    err.append("\nTotal kmer nodes number:    %d\n" % total)
    for label, v in (("Deleted lowfreq kmer nodes: ", deleted), ("Used linear kmer nodes:     ", linear), ("Used tip kmer nodes:        ", len(tips)),
                     ("Used branching kmer nodes:  ", len(branches))):
        err.append("%s%d\t%s\n" % (label, v, fmt_double(v / total)))
    if o.T:
        files["tip.fa"] = remove_tips(t, o, tips, err).encode()
    if o.W:
        files["lowedge.fa"] = remove_low_edges(t, o, branches, err).encode()
    if o.B:
        files["bubble.fa"] = remove_bubbles(t, o, branches, err).encode()
    contigs = read_out_contigs(t)
    files["seq.fa"], files["seq.depth"], files["small.fa"], files["small.depth"] = contig_files(t, o, contigs, err)
    return files, "".join(err), contigs
