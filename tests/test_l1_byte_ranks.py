"""GPU (-m gpu): the pipelined level 1 with ranks counted in bytes and the bucket word that carries the histogram entry's place
(L1Pipe, dbgk_partition_l1.h), at the smallest shapes at which that encoding can go wrong.  Every case builds the same reads twice --
through the PARTITION engine and through the atomic engine (DIRECT: global atomics on one table, no records, no LDS staging; for
KFREQ the atomic counting path) -- and compares node count, k-mer total, node digest, DepthStat and the key-0 node's links, as
bench.py's verify_single does; the KFREQ case compares the counter table byte for byte.

  rank field at its maximum   2 048 identical reads of 150 x C, k = 31: sixteen regular tiles whose 15 360 records all land in one
                              bucket (ranks up to 15 359 records = 122 872 bytes), with room for them in the bucket
  a bucket that fills         the same reads on a handle that expects only the batch's own size: the bucket's capacity is exceeded, the
                              runs go out record by record (copy_slow) and into the overflow list, under the scaled counts
  zero key and dummy bins     the same tile count, 150 x A reads mixed 1 : 7 among random reads: the zero key, the dummy bins, staging
                              record by record (the path that tests for "has no bucket")
  tile counts                 random reads, 128 * 3 + 5 (three regular tiles, then the general form and the last tile's copy_rest), 127
                              (no regular tile), 128 (exactly one)
  table sizes                 2^26 slots, the smallest the engine accepts (the planner gives it 64 level-1 buckets: the straight-line
                              scan's first lanes), 600 000 001 slots (144 buckets: its upper lanes), and 257 buckets (the loop scan)
  other forms                 k = 17 (nine lanes per read: the general equal-length form) and k = 32 at 150 bases, 151-base reads at
                              k = 31 (lanes partly filled), mixed lengths in 60 .. 150 (the lane-prefix form), and a KFREQ handle with
                              direct blocks at k = 13 (32-bit records, ranks in units of 4, sixteen windows per lane)
"""
import numpy as np
import pytest

READ_LEN, K = 150, 31
SMALLEST = 1 << 26
CFG2_LIKE = 600000001


def _ascii(codes):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[codes]


def _random_reads(n, length, seed):
    return [_ascii(r) for r in np.random.default_rng(seed).integers(0, 4, size=(n, length))]


def _same(n, base, length=READ_LEN):
    return [np.full(length, ord(base), dtype=np.uint8) for _ in range(n)]


def _batch(reads):
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads), offsets


def _summary(g, st):
    return (int(st.total_reads), int(st.total_kmers), int(st.count), int(st.stored_kmers), g.digest(),
            [int(x) for x in g.link_stats(2).depth_stat], int(st.polyA_l_link), int(st.polyA_r_link))


def _compare(reads, size, k=K, expected=None, n1=None, uniform=True, want_launch="uniform_launches"):
    """the PARTITION engine (packed input; equal lengths without offsets, as the benchmark pushes them) against the atomic engine"""
    from dbg_assembly_amd import capi
    bases, offsets = _batch(reads)
    words, other = capi.pack_bases(bases)
    assert other == 0
    expected = len(bases) if expected is None else expected
    if n1 is not None:
        assert capi.plan_partition(size, expected).level1_buckets == n1, (size, capi.plan_partition(size, expected).level1_buckets)
    with capi.Graph(k=k, table_slots=size, max_read_len=250, engine=capi.ENGINE_PARTITION, expected_kmers=expected) as g:
        if uniform:
            g.push_reads_packed_uniform(words, len(reads), len(reads[0]), 0)
        else:
            g.push_reads_packed(words, offsets, 0)
        st = g.finalize()
        assert getattr(g.timings(), want_launch) >= 1, "the batch did not take the form under test"
        got = _summary(g, st)
    with capi.Graph(k=k, table_slots=size, max_read_len=250, engine=capi.ENGINE_DIRECT, expected_kmers=0) as v:
        v.push_reads(bases, offsets)
        want = _summary(v, v.finalize())
    print("count %d  k-mers %d  digest %016x" % (got[2], got[3], got[4]))
    assert got == want
    return got


@pytest.mark.gpu
def test_rank_field_at_its_maximum():
    reads = _same(2048, "C")
    # room for the 245 760 records of the one bucket: a handle that expects 64 buckets' worth of them
    got = _compare(reads, SMALLEST, expected=64 * 250000, n1=64)
    assert got[3] == 2048 * 120


@pytest.mark.gpu
def test_a_bucket_that_fills():
    reads = _same(2048, "C")
    got = _compare(reads, SMALLEST, n1=64)   # capacity of a bucket: 307 200 / 64 + 64 K records, far below 245 760
    assert got[3] == 2048 * 120


@pytest.mark.gpu
def test_zero_key_and_dummy_bins():
    reads = _random_reads(2048, READ_LEN, 41)
    for i in range(0, 2048, 8):
        reads[i] = np.full(READ_LEN, ord("A"), dtype=np.uint8)
    got = _compare(reads, SMALLEST, n1=64)
    assert got[6] or got[7], "no key-0 links: the poly-A reads were not seen"


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", (128 * 3 + 5, 127, 128))
def test_tile_counts_around_the_remainder_kernel(n_reads):
    _compare(_random_reads(n_reads, READ_LEN, 42), SMALLEST, n1=64)


@pytest.mark.gpu
def test_table_with_144_buckets():
    _compare(_random_reads(128 * 3 + 5, READ_LEN, 43), CFG2_LIKE, n1=144)


@pytest.mark.gpu
def test_table_with_257_buckets_loop_scan():
    from dbg_assembly_amd import capi
    n_bases = (128 * 3 + 5) * READ_LEN
    size = next(s for s in (capi.find_next_prime_ref((257 << 22) - 4000), 257 << 22) if capi.plan_partition(s, n_bases).level1_buckets == 257)
    _compare(_random_reads(128 * 3 + 5, READ_LEN, 44), size, n1=257)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (17, 32))
def test_other_k_at_150_bases(k):
    _compare(_random_reads(128 * 3 + 5, READ_LEN, 45), SMALLEST, k=k)


@pytest.mark.gpu
def test_151_base_reads_partly_filled_lanes():
    _compare(_random_reads(128 * 3 + 5, 151, 46), SMALLEST)


@pytest.mark.gpu
def test_mixed_lengths_take_the_prefix_form():
    rng = np.random.default_rng(47)
    reads = [_ascii(rng.integers(0, 4, size=int(n))) for n in rng.integers(60, 151, size=128 * 3 + 5)]
    reads[0], reads[-1] = reads[0][:60], _ascii(rng.integers(0, 4, size=150))   # (both ends of the range are there)
    reads[7] = np.full(150, ord("A"), dtype=np.uint8)
    _compare(reads, SMALLEST, uniform=False, want_launch="prefix_launches")


@pytest.mark.gpu
def test_kfreq_direct_blocks_k13_equals_atomic_counts():
    from dbg_assembly_amd import capi
    k = 13
    reads = _random_reads(128 * 3 + 5, READ_LEN, 48) + _same(300, "C") + _same(40, "A")
    bases, offsets = _batch(reads)
    words, other = capi.pack_bases(bases)
    assert other == 0
    n_kmers = len(reads) * (READ_LEN - k + 1)
    with capi.Graph(k=k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000000, expected_kmers=n_kmers) as g:
        g.push_reads_packed_uniform(words, len(reads), READ_LEN, 0)
        st = g.finalize()
        assert g.timings().uniform_launches >= 1, "the batch did not take the equal-length form"
        got, got_total = g.kfreq_counts(), int(st.stored_kmers)
    with capi.Graph(k=k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000000, expected_kmers=0) as v:
        v.push_reads(bases, offsets)
        st = v.finalize()
        assert v.timings().uniform_launches == 0
        want, want_total = v.kfreq_counts(), int(st.stored_kmers)
    assert got_total == want_total == n_kmers
    assert int(want.max()) == 255 and np.array_equal(got, want)
