"""GPU steps of tests/test_wide_links_gpu.py, each run in a child process of its own under a time limit:
    python tests/wide_links_gpu_steps.py shapes | placed | anchor
The WIDE engine's table together with the contig stage's first pass (dbgk_wide_export_host_table_links: k_wide_kmer_links on the
device table, the nodes placed on the host patched in) against contig_restatement.first_pass applied to the array and flags the same
call returned, slot for slot.  PARITY UNPINNED above k = 32; `anchor` ties the pass to the 64-bit one at k = 31.  Also the reads of
the `placed` step and of the command-line tests (placed_reads), which tests/test_wide_links_cpu.py checks without a GPU.  Prints one
JSON line of findings; exits non-zero on a mismatch."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
import wide_contig_restatement as W  # noqa: E402

KS = (33, 48, 63)
CUTOFFS = (0, 2, 5)
BLOCK_SLOTS = 4096   # kLinkChunk: the slots one block of k_wide_kmer_links owns
PLACED_SIZE = 30011  # the table of `-i 0.00003`


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def placed_reads(k):
    """W.cli_reads() plus reads whose first k-mer has a zero low word (it ends in 32 A's) and is canonical, so that the node lives in
    the device's side table and is put on its chain by the host: one that is a tip, one that is a branch, one deleted at cutoff 2;
    reads that make the key-0 node a live node; one read 300 times (counters at 255); four reads that share k bases and go on with
    A, C, G and T (a side with four links)"""
    rng = random.Random(500 + k)
    pre, a32 = rand_seq(rng, k - 33), "A" * 32
    tail, tail2, tail3 = rand_seq(rng, 40), rand_seq(rng, 40), rand_seq(rng, 40)
    reads = list(W.cli_reads()[1])
    reads += [pre + "C" + a32 + "G" + tail] * 5
    reads += [pre + "G" + a32 + "C" + tail2] * 5 + [pre + "G" + a32 + "T" + tail3] * 5
    reads += [pre + "T" + a32 + "C" + tail] * 1
    reads += ["A" * (k + 7) + "C" + tail] * 5
    reads += [rand_seq(rng, 100)] * 300
    shared = rand_seq(rng, k)
    reads += [shared + b + rand_seq(rng, 30) for b in "ACGT"] * 3
    return reads


def shape_reads(rng, k, size):
    """a genome that fills a third of the table, tiled by reads three times over, and variants of single reads (one substitution,
    three copies or one): tips at the ends, branches at the variants, counters on both sides of every cutoff tried"""
    genome = rand_seq(rng, size // 3 + k)
    step = 150 - k - 20
    tiles = [genome[p:p + 150] for p in range(0, max(len(genome) - k, 1), step)]
    reads = tiles * 3 + tiles[::2] * 4
    for v in range(max(1, size // 400)):
        r = list(tiles[0] if v == 0 else rng.choice(tiles))
        p = rng.randrange(k, len(r) - k) if v == 0 else rng.randrange(len(r))   # the first one k bases from both ends: a bubble, two branches
        r[p] = rng.choice([b for b in "ACGT" if b != r[p]])
        reads += ["".join(r)] * (1 if v % 2 else 3)   # (seen once: a link that only cutoff 0 counts)
    return [r for r in reads if len(r) >= k]


def pack(reads):
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    offsets = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return bases, offsets


def table_of(k, array, flags, cls=W.WideTable):
    size = len(array)
    t = cls(size, k)
    for i in np.flatnonzero(np.unpackbits(flags)[:size]):
        i = int(i)
        t.kmer[i], t.l_link[i], t.r_link[i], t.filled[i] = (int(array["kmer_hi"][i]) << 64) | int(array["kmer_lo"][i]), int(array["l_link"][i]), int(array["r_link"][i]), True
    return t


def stats_words(ls):
    return list(ls.depth_stat) + [ls.total_nodes, ls.deleted_lowfreq, ls.linear_nodes, ls.tip_nodes, ls.branch_nodes]


def compare(what, k, cutoff, result):
    """the seven results of wide_export_host_table_links against first_pass on the table among them -> the table, after first_pass"""
    array, flags, klink, dele, tips, branches, ls = result
    t = table_of(k, array, flags)
    want_tips, want_branches, stat, (total, deleted, linear) = R.first_pass(t, R.Options(D=cutoff))
    _, want_flags, want_del, want_klink = t.arrays()
    assert np.array_equal(flags, want_flags), (what, "nul_flag")
    assert np.array_equal(klink, want_klink), (what, "klink", np.flatnonzero(klink != want_klink)[:8].tolist())
    assert np.array_equal(dele, want_del), (what, "del_flag")
    assert tips.tolist() == want_tips, (what, "tips", len(tips), len(want_tips))
    assert branches.tolist() == want_branches, (what, "branches", len(branches), len(want_branches))
    assert np.all(np.diff(tips.astype(np.int64)) > 0) and np.all(np.diff(branches.astype(np.int64)) > 0), (what, "ascending")
    want_stats = stat + [total, deleted, linear, len(want_tips), len(want_branches)]
    assert len(want_stats) == 261 and stats_words(ls) == want_stats, (what, "stats")
    return t


def raw_call(g, size, cutoff, tip_cap, branch_cap, with_lists=True):
    """the C call itself, with capacities of the caller's choosing -> status, n_tips, n_branches, the two buffers"""
    from dbg_assembly_amd import capi
    array, flags = np.zeros(size, dtype=capi.NODE32_DTYPE), np.zeros(size // 8 + 1, dtype=np.uint8)
    klink, dele = np.zeros(size, dtype=np.uint16), np.zeros(size // 8 + 1, dtype=np.uint8)
    tips, branches = np.full(tip_cap + 1, 2 ** 64 - 1, dtype=np.uint64), np.full(branch_cap + 1, 2 ** 64 - 1, dtype=np.uint64)
    nt, nb = C.c_uint64(), C.c_uint64()
    rc = capi.lib().dbgk_wide_export_host_table_links(g._h, size, array.ctypes.data, flags.ctypes.data, cutoff, klink.ctypes.data, dele.ctypes.data,
                                                      tips.ctypes.data if with_lists else None, tip_cap, C.byref(nt),
                                                      branches.ctypes.data if with_lists else None, branch_cap, C.byref(nb), None)
    return rc, nt.value, nb.value, tips, branches


def check_refusals(g, size):
    """null klink / del_flag / n_tips / n_branches: DBGK_ERR_ARG; a handle that is not WIDE and a shard of a WIDE table: DBGK_ERR_STATE"""
    from dbg_assembly_amd import capi
    L = capi.lib()
    array, flags = np.zeros(size, dtype=capi.NODE32_DTYPE), np.zeros(size // 8 + 1, dtype=np.uint8)
    klink, dele = np.zeros(size, dtype=np.uint16), np.zeros(size // 8 + 1, dtype=np.uint8)
    nt, nb = C.c_uint64(), C.c_uint64()

    def call(h, **null):
        a = dict(klink=klink.ctypes.data, dele=dele.ctypes.data, nt=C.byref(nt), nb=C.byref(nb))
        a.update(null)
        return L.dbgk_wide_export_host_table_links(h, size, array.ctypes.data, flags.ctypes.data, 2, a["klink"], a["dele"], None, 0, a["nt"], None, 0, a["nb"], None)

    for name in ("klink", "dele", "nt", "nb"):
        assert call(g._h, **{name: None}) == capi.ERR_ARG, name
    assert not array["kmer_lo"].any() and not flags.any()   # nothing was written
    assert call(g._h) == 0
    with capi.Graph(k=31, table_slots=size, max_read_len=150, engine=capi.ENGINE_DIRECT, device=0) as narrow:
        narrow.finalize()
        assert call(narrow._h) == capi.ERR_STATE
    big = capi.find_next_prime_ref(1 << 26)
    with capi.Graph(k=63, table_slots=big, engine=capi.ENGINE_WIDE, expected_kmers=1 << 20, shard_count=2, shard_index=0, max_read_len=150, device=0) as shard:
        assert call(shard._h) == capi.ERR_STATE


def step_shapes():
    """sizes that reach each boundary of the kernel: less than one sweep of 256 threads with a partial last del_flag byte, three slots
    into a second block, three blocks and more at a size that is no multiple of 8 or 64"""
    from dbg_assembly_amd import capi
    out = {}
    for k in KS:
        for size in (251, 4099, 12301):
            assert size % 8 and size % 64
            rng = random.Random(k * 100000 + size)
            bases, offsets = pack(shape_reads(rng, k, size))
            with capi.Graph(k=k, table_slots=size, max_read_len=150, engine=capi.ENGINE_WIDE, device=0) as g:
                g.push_reads(bases, offsets)
                st = g.finalize()
                assert size // 4 < st.count < size
                if (k, size) == (63, 251):
                    check_refusals(g, size)
                for cutoff in CUTOFFS:
                    what = "k %d size %d cutoff %d" % (k, size, cutoff)
                    res = g.wide_export_host_table_links(cutoff, size)
                    compare(what, k, cutoff, res)
                    tips, branches = res[4], res[5]
                    out[what] = [len(tips), len(branches), int(res[6].deleted_lowfreq)]
                    if cutoff == 2:
                        assert len(tips) > 0 and len(branches) > 0, (what, len(tips), len(branches))
                        if size > 3 * BLOCK_SLOTS:   # list entries from more than one block
                            assert len({int(i) // BLOCK_SLOTS for i in tips}) > 1 and len({int(i) // BLOCK_SLOTS for i in branches}) > 1, what
                        # capacities exactly sufficient, one short each, and no list pointers: counts only
                        rc, nt, nb, a, b = raw_call(g, size, cutoff, len(tips), len(branches))
                        assert (rc, nt, nb) == (0, len(tips), len(branches)) and a[:nt].tolist() == tips.tolist() and b[:nb].tolist() == branches.tolist()
                        assert a[nt] == 2 ** 64 - 1 and b[nb] == 2 ** 64 - 1   # nothing behind the capacity
                        for tc, bc in ((len(tips) - 1, len(branches)), (len(tips), len(branches) - 1)):
                            rc, nt, nb, a, b = raw_call(g, size, cutoff, tc, bc)
                            assert (rc, nt, nb) == (capi.ERR_CAPACITY, len(tips), len(branches)), (what, rc, nt, nb)
                        rc, nt, nb, _, _ = raw_call(g, size, cutoff, 0, 0, with_lists=False)
                        assert (rc, nt, nb) == (0, len(tips), len(branches)), (what, rc, nt, nb)
    return out


def placed_conditions(results):
    """results: {(k, cutoff): (table after first_pass, tips, branches)} -> what the crafted reads are there for, as assertions"""
    inner = {"tips": False, "branches": False}
    for (k, cutoff), (t, tips, branches) in results.items():
        zero_low = lambda i: t.kmer[i] & W.M64 == 0   # noqa: E731
        zt, zb = [i for i in tips if zero_low(i)], [i for i in branches if zero_low(i)]
        if cutoff in (0, 2):
            assert zt and zb, (k, cutoff, "a tip and a branch with a zero low word", zt, zb)
        inner["tips"] |= any(i not in (tips[0], tips[-1]) for i in zt)
        inner["branches"] |= any(i not in (branches[0], branches[-1]) for i in zb)
        for name, lst in (("tips", tips), ("branches", branches)):
            if cutoff in (0, 2):
                assert len({i // BLOCK_SLOTS for i in lst}) > 1, (k, cutoff, name, "one block only")
    assert inner["tips"] and inner["branches"], inner   # not only at the first or last position for every k and cutoff tried


def step_placed():
    from dbg_assembly_amd import capi
    out, results = {}, {}
    for k in KS:
        bases, offsets = pack(placed_reads(k))
        with capi.Graph(k=k, table_slots=PLACED_SIZE, max_read_len=150, engine=capi.ENGINE_WIDE, device=0) as g:
            g.push_reads(bases, offsets)
            g.finalize()
            for cutoff in CUTOFFS:
                res = g.wide_export_host_table_links(cutoff, PLACED_SIZE)
                t = compare("placed k %d cutoff %d" % (k, cutoff), k, cutoff, res)
                results[(k, cutoff)] = (t, res[4].tolist(), res[5].tolist())
                slot0 = next(i for i in range(t.size) if t.filled[i] and t.kmer[i] == 0)
                assert not t.deleted[slot0]   # the key-0 node is a live node: a branch, and linear at cutoff 5
                assert (slot0 in res[5].tolist()) == (cutoff < 5) and bool(t.linear[slot0]) == (cutoff == 5)
                assert list(res[6].depth_stat)[255] > 0
                out["k%d_D%d" % (k, cutoff)] = [len(res[4]), len(res[5]), sum(1 for i in range(t.size) if t.filled[i] and t.kmer[i] & W.M64 == 0)]
    placed_conditions(results)
    return out


def step_anchor():
    """k = 31: the wide engine and a narrow handle on the same reads at the same table size.  Slots of colliding keys may differ (the
    two hash the same, but claim slots in another order), so records, delete bits and list membership are compared by k-mer"""
    from dbg_assembly_amd import capi
    out = {}
    for name, cutoff in (("b_tips", 1), ("d_bubbles", 2)):
        c = R.load_case(os.path.join(ROOT, "tests", "golden", "contig_cases", name + ".npz"))
        assert c["k"] == 31
        reads = [ln for ln in c["reads"].decode().split("\n") if ln and not ln.startswith(">")]
        bases, offsets = pack(reads)
        size = int(c["table_size"])
        with capi.Graph(k=31, table_slots=size, max_read_len=150, engine=capi.ENGINE_DIRECT, device=0) as g:
            g.push_reads(bases, offsets)
            g.finalize()
            n_array, n_flags, n_klink, n_del, n_tips, n_branches, n_ls = g.export_host_table_links(cutoff, size)
        with capi.Graph(k=31, table_slots=size, max_read_len=150, engine=capi.ENGINE_WIDE, device=0) as g:
            g.push_reads(bases, offsets)
            g.finalize()
            res = g.wide_export_host_table_links(cutoff, size)
        compare("anchor " + name, 31, cutoff, res)
        w_array, w_flags, w_klink, w_del, w_tips, w_branches, w_ls = res
        assert not w_array["kmer_hi"].any()

        def by_kmer(kmers, flags, klink, dele, tips, branches):
            occ = np.flatnonzero(np.unpackbits(flags)[:size])
            dbits, tset, bset = np.unpackbits(dele)[:size], set(tips.tolist()), set(branches.tolist())
            return {int(kmers[i]): (int(klink[i]), int(dbits[i]), int(i) in tset, int(i) in bset) for i in occ}

        narrow = by_kmer(n_array["kmer"], n_flags, n_klink, n_del, n_tips, n_branches)
        wide = by_kmer(w_array["kmer_lo"], w_flags, w_klink, w_del, w_tips, w_branches)
        assert narrow == wide, name
        assert stats_words(n_ls) == stats_words(w_ls)
        assert np.all(np.diff(w_tips.astype(np.int64)) > 0) and np.all(np.diff(w_branches.astype(np.int64)) > 0)
        assert len(w_tips) > 0 and len(w_branches) > 0
        out[name] = [len(w_tips), len(w_branches)]
    return out


if __name__ == "__main__":
    res = {"shapes": step_shapes, "placed": step_placed, "anchor": step_anchor}[sys.argv[1]]()
    print(json.dumps(res))
