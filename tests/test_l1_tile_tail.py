"""GPU (-m gpu): the per-tile part of the pipelined level 1 (L1Pipe::tail and the decode in front of the positions) at the bucket
counts where its code changes.

Behind the positions of a tile every wave scans the tile's histogram for itself.  Up to 256 level-1 buckets the scan is straight-line
code -- lane l owns buckets 4 l .. 4 l + 3 whatever the bucket count, buckets beyond n1 read zero -- and above it the loop over
E = ceil(n1 / 64) buckets per lane.  What can go wrong is a bucket whose first staged index is off (its records land in the
neighbour's run: wrong slots, lost or doubled nodes), at the last bucket of a lane's group or past the last lane that owns any: n1 =
64, 65, 128, 129, 144 (the benchmark's table), 192, 193, 256 and 257 are E = 1 .. 4 at both edges, and the first count that keeps
the loop (E = 5).  n1 comes from dbgk_plan_partition and is asserted: a change of the planner cannot silently move a case.

Input: 300 reads of 150 bases, k = 31 -- two whole tiles of 128 reads (regular tiles, 15 windows per lane, every lane full) and 44
reads that take the general equal-length form.  Against the oracle: sorted node dump, counts, the key-0 node.  The tables are
written once by the region build and never zeroed, so even the largest (1.08 G slots) costs milliseconds.  At n1 = 64 and 144 the
other forms that share the tail run too: ASCII with offsets, the lane-prefix form (a few reads trimmed), a read with k times A (one
wave stages record by record in a tile whose other waves take the path without a test), and -- once, its bucket count is set by k
alone -- a KFREQ handle at k = 17 with direct blocks (32-bit records)."""
import random

import numpy as np
import pytest

from helpers import set_hooks

READ_LEN, N_READS, K = 150, 300, 31
N1S = (64, 65, 128, 129, 144, 192, 193, 256, 257)
N1_LINEAR_ABOVE = 320   # (kL1LinearAboveN1, dbgk_l1_form.h) tables with more level-1 buckets take the linear form


def _reads(seed, with_poly_a=False):
    rng = random.Random(seed)
    reads = []
    while len(reads) < N_READS:
        r = "".join(rng.choice("ACGT") for _ in range(READ_LEN))
        if not any(b * 16 in r for b in "ACGT"):
            reads.append(r)
    if with_poly_a:   # read 70 (tile 0): K times A from base 40 on, a different base on either side
        r = list(reads[70])
        r[39:41 + K] = "C" + "A" * K + "C"
        reads[70] = "".join(r)
    return [r.encode() for r in reads]


def _table_for(capi, n1, expected):
    """the smallest table the planner gives n1 level-1 buckets: a prime just below n1 << r, or n1 << r itself"""
    for r in (20, 21, 22):
        for size in (capi.find_next_prime_ref((n1 << r) - 4000), n1 << r):
            if (1 << 26) <= size <= (n1 << r) and capi.plan_partition(size, expected).level1_buckets == n1:
                return size
    raise AssertionError("no table size plans to %d level-1 buckets" % n1)


@pytest.fixture(scope="module")
def plain(oracle):
    from dbg_assembly_amd import capi
    reads = _reads(31)
    bases, offsets = oracle.pack_reads(reads)
    words, other = capi.pack_bases(bases)
    assert other == 0
    ref = oracle.build_graph(files_mem=[(bases, offsets)], k=K, max_read_len=250, init_hash_size=0.001, threads=1)
    return bases, offsets, words, ref, ref.nodes.astype(capi.NODE_DTYPE)


def _check(g, st, ref, want, what):
    assert (st.total_reads, st.total_kmers, st.count) == (ref.total_reads, ref.total_kmers, ref.count), what
    assert np.array_equal(g.export_sorted(), want), what
    assert (st.polyA_l_link, st.polyA_r_link) == (int(want[0]["l_link"]), int(want[0]["r_link"])), what


def _graph(capi, n1, n_bases):
    size = _table_for(capi, n1, n_bases)
    plan = capi.plan_partition(size, n_bases)
    assert plan.level1_buckets == n1, (size, plan.level1_buckets)
    return capi.Graph(k=K, table_slots=size, max_read_len=250, engine=capi.ENGINE_PARTITION, expected_kmers=n_bases)


@pytest.mark.gpu
@pytest.mark.parametrize("n1", N1S)
def test_regular_tiles_equal_oracle_at_n1(plain, n1):
    from dbg_assembly_amd import capi
    bases, offsets, words, ref, want = plain
    assert n1 <= N1_LINEAR_ABOVE, "the planner's threshold: this bucket count takes the wave-per-bucket form, whose tail is under test"
    with _graph(capi, n1, len(bases)) as g:
        g.push_reads_packed_uniform(words, N_READS, READ_LEN, 0)
        st = g.finalize()
        assert g.timings().uniform_launches >= 1, "the batch did not take the equal-length form"
        _check(g, st, ref, want, n1)


@pytest.mark.gpu
@pytest.mark.parametrize("n1", (64, 144))
def test_ascii_with_offsets_equals_oracle(plain, n1):
    """the general equal-length form (ASCII packed on the way into LDS, 64-bit read offsets)"""
    from dbg_assembly_amd import capi
    bases, offsets, words, ref, want = plain
    with _graph(capi, n1, len(bases)) as g:
        g.push_reads(bases, offsets)
        st = g.finalize()
        _check(g, st, ref, want, n1)


@pytest.mark.gpu
@pytest.mark.parametrize("n1", (64, 144))
def test_prefix_form_equals_oracle(oracle, monkeypatch, n1):
    """a few reads trimmed to 60 .. 149 bases: the lane-prefix form (partly filled lanes, record-by-record staging)"""
    from dbg_assembly_amd import capi
    reads = _reads(32)
    rng = random.Random(5)
    for rd in rng.sample(range(N_READS), 25):
        reads[rd] = reads[rd][:rng.randint(60, 149)]
    bases, offsets = oracle.pack_reads(reads)
    words, other = capi.pack_bases(bases)
    ref = oracle.build_graph(files_mem=[(bases, offsets)], k=K, max_read_len=250, init_hash_size=0.001, threads=1)
    want = ref.nodes.astype(capi.NODE_DTYPE)
    set_hooks(monkeypatch, l1_prefix="1")
    with _graph(capi, n1, len(bases)) as g:
        g.push_reads_packed(words, offsets, other)
        st = g.finalize()
        assert g.timings().prefix_launches >= 1, "the batch did not take the prefix form"
        _check(g, st, ref, want, n1)


@pytest.mark.gpu
@pytest.mark.parametrize("n1", (64, 144))
def test_one_wave_with_a_zero_key_equals_oracle(oracle, n1):
    """one read carries K times A: its wave keeps the per-position test and stages record by record, the tile's other waves do not"""
    from dbg_assembly_amd import capi
    reads = _reads(33, with_poly_a=True)
    bases, offsets = oracle.pack_reads(reads)
    words, other = capi.pack_bases(bases)
    assert other == 0
    ref = oracle.build_graph(files_mem=[(bases, offsets)], k=K, max_read_len=250, init_hash_size=0.001, threads=1)
    want = ref.nodes.astype(capi.NODE_DTYPE)
    assert want[0]["kmer"] == 0 and (int(want[0]["l_link"]) or int(want[0]["r_link"])), "the oracle saw no key 0"
    with _graph(capi, n1, len(bases)) as g:
        g.push_reads_packed_uniform(words, N_READS, READ_LEN, 0)
        st = g.finalize()
        _check(g, st, ref, want, n1)


@pytest.mark.gpu
def test_kfreq_direct_blocks_k17_equals_sparse_restatement(oracle, plain):
    """32-bit records through the same tail.  A KFREQ handle's level-1 buckets are set by k alone (k = 17: 4^17 >> 26 = 256, the last
    straight-line count), so this runs once.  Checked on the device over the whole table (the spectrum of the counters) and value
    by value over its first 2^26 counters."""
    from dbg_assembly_amd import capi
    k = 17
    bases, offsets = plain[0], plain[1]
    raw = np.ascontiguousarray(bases, dtype=np.uint8).tobytes()
    parts = [oracle.parse_read(raw[int(offsets[i]):int(offsets[i + 1])], k, 1000)[0] for i in range(len(offsets) - 1)]
    allk = np.concatenate(parts)
    uniq, cnt = np.unique(allk, return_counts=True)
    uniq, cnt = uniq.astype(np.uint64), np.minimum(cnt, 255).astype(np.uint8)
    with capi.Graph(k=k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000000, expected_kmers=len(allk)) as g:
        words, other = capi.pack_bases(bases)
        g.push_reads_packed_uniform(words, N_READS, READ_LEN, other)
        st = g.finalize()
        assert g.timings().uniform_launches >= 1, "the batch did not take the equal-length form"
        assert (int(st.count), int(st.stored_kmers)) == (len(uniq), len(allk))
        spectrum = g.kfreq_spectrum()
        want = np.bincount(cnt, minlength=256).astype(np.uint64)
        want[0] = 4 ** k - len(uniq)
        assert np.array_equal(spectrum, want)
        span = 1 << 26
        got = g.kfreq_counts(0, span)
        hi = int(np.searchsorted(uniq, span))
        assert hi > 0 and int(np.count_nonzero(got)) == hi
        assert np.array_equal(got[uniq[:hi].astype(np.int64)], cnt[:hi])
