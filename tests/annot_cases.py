"""Crafted batches for the annotation kernels (csrc/dbgk_annot.h): records of a corrector with the lengths of their reads, at the
shapes where a length pass, a scan and a grouped write through LDS can go wrong.  A case is {"rec": REC_DTYPE[n], "L": read
lengths}; the reads themselves are bytes of 'A' (the annotation does not look at them).  `expected` is the restatement
(tests/annot_restatement.py) on the compact lengths of tests/corr_compact_restatement.py.

What the device cannot be given: a compact length of 10^8 and more needs a read of 100 MB, one of 10^9 a read longer than the
2^29 bytes the corrector takes; so F reaches 8 digits on the GPU, and CPU_ONLY holds the records whose F is longer -- the
longest of them is the bound DBGK_CORR_ANNOT_MAX -- for the restatement alone."""
import numpy as np

import annot_restatement as AR
import corr_compact_restatement as CC

GROUP = 256        # records per workgroup round of k_annot_write (kAnnotGroup)
BOUNDARIES = [0, 9] + [v for p in range(1, 10) for v in (10 ** p, 10 ** (p + 1) - 1)][:-1] + [4294967295]   # 0 9 10 99 100 ... 999999999 1000000000 2^32-1
F_BOUNDARIES = [v for v in BOUNDARIES if v <= 10 ** 7]
D_VALUES = [0, 1, 9, 10, 99, 100, 255]
MIN_SUFFIX = sum(len(x) for x in AR.LITERALS) + 5


def case(rows, L):
    """rows: (one_base, tree, left_trim, right_trim, deleted) per record; L: the length of every read, or one per record"""
    rec = np.zeros(len(rows), dtype=CC.REC_DTYPE)
    for i, r in enumerate(rows):
        rec[i]["one_base"], rec[i]["tree"], rec[i]["left_trim"], rec[i]["right_trim"], rec[i]["deleted"] = r
    rec["node_limit_hits"] = 0xDEAD   # (not printed)
    return {"rec": rec, "L": np.full(len(rows), L, dtype=np.uint64) if np.isscalar(L) else np.asarray(L, dtype=np.uint64)}


def batch(c):
    """-> (bases uint8, offsets uint64[n + 1]) as Corrector.compact_from takes them"""
    off = np.zeros(len(c["L"]) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(c["L"])
    return np.full(max(int(off[-1]), 1), ord("A"), dtype=np.uint8), off


def compact_lengths(c):
    return CC.out_lengths(batch(c)[1], c["rec"])


def expected(c):
    """-> (suffix bytes uint8, offsets uint64[n + 1])"""
    return AR.suffixes(c["rec"], c["F"] if "F" in c else compact_lengths(c))


def mixed(n, seed):
    """n records whose five numbers have every digit count, reads of 0 .. 120 bytes"""
    rng = np.random.RandomState(seed)
    rows, L = [], []
    for _ in range(n):
        v = [int(rng.randint(0, 10 ** int(rng.randint(1, 11)))) & 0xFFFFFFFF for _ in range(4)]
        if rng.rand() < 0.6:
            v[2] %= 40
            v[3] %= 40   # (a kept read with a length to print)
        rows.append((v[0], v[1], v[2], v[3], int(rng.rand() < 0.2) * int(rng.choice(D_VALUES[1:]))))
        L.append(int(rng.randint(0, 121)))
    return case(rows, L)


def of_total(total):
    """records of one digit per number, the first ones given more digits, so that the suffix bytes total exactly `total`"""
    n = total // MIN_SUFFIX
    extra = total - n * MIN_SUFFIX
    rows = []
    for _ in range(n):
        d = [min(9, max(0, extra - 9 * j)) for j in range(3)]   # digits added to M, Lt, Rt
        extra -= sum(d)
        rows.append((10 ** d[0] if d[0] else 0, 0, 10 ** d[1] if d[1] else 0, 10 ** d[2] if d[2] else 0, 0))
    assert extra == 0
    return case(rows, 5)


def cases():
    out = {}
    rows = []
    for v in BOUNDARIES:
        rows += [(v, 0, 0, 0, 0), (0, v, 0, 0, 0), (0, 0, v, 0, 0), (0, 0, 0, v, 0), (v, 0, v, v, 0)]
    out["every_digit_boundary_M_Lt_Rt"] = case(rows, 5)
    out["every_digit_boundary_F"] = case([(0, 0, 0, 0, 0)] * len(F_BOUNDARIES) + [(0, 0, 3, 4, 0)] * len(F_BOUNDARIES),
                                         F_BOUNDARIES + [v + 7 for v in F_BOUNDARIES])
    out["every_digit_boundary_D"] = case([(1, 2, 0, 0, d) for d in D_VALUES], 30)
    out["sum_that_wraps"] = case([(4294967295, 1, 0, 0, 0), (1 << 31, 1 << 31, 0, 0, 0), (4294967290, 10, 0, 0, 0), (4294967295, 4294967295, 0, 0, 0)], 9)
    out["deleted"] = case([(3, 4, 5, 6, 1), (0, 0, 0, 0, 1), (1, 1, 100, 100, 1), (7, 0, 0, 0, 0)], 100)
    out["trims_that_meet_or_pass_the_read"] = case([(0, 0, 50, 50, 0), (0, 0, 100, 0, 0), (0, 0, 0, 100, 0), (0, 0, 60, 41, 0), (0, 0, 4294967295, 4294967295, 0),
                                                    (0, 0, 50, 49, 0)], 100)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 2 * GROUP - 1, 2 * GROUP, 2 * GROUP + 1):
        out["n_%d" % n] = mixed(n, 1000 + n)
    for extra in (0, 1):
        out["suffix_bytes_16384%+d" % extra] = of_total(16384 + extra)
    out["all_minimal"] = case([(0, 0, 0, 0, 0)] * 1000, 5)
    # the longest suffixes records on the device can give: F has one digit when both trims have ten
    out["all_maximal"] = case([(4294967295, 0, 4294967295, 4294967295, 255)] * (2 * GROUP + 88), 5)
    out["large"] = mixed(20000, 7)
    out["small_after_large"] = mixed(3, 8)
    return out


# for the restatement alone: compact lengths no device batch reaches
CPU_ONLY = dict(case([(4294967295, 0, 4294967295, 4294967295, 255), (0, 0, 0, 0, 0), (1, 1, 1, 1, 1)], 5), F=[4294967295, 10 ** 8, 999999999])
