"""GPU (-m gpu): level 1 tests for the zero key once per wave and tile (k >= 31) instead of once per position.

A canonical key is 0 only for a window of k times A / N or k times T, and such a run covers a whole aligned packed word of 16
bases: a wave whose lanes funnel their windows from no word 0x00000000 / 0xFFFFFFFF runs the positions without the test
(l1_positions<..., ZERO_POSSIBLE = false>), every other wave the positions with it.  The detection is conservative, so what can go
wrong is a key-0 window the per-wave test does not see (the record of key 0 would land in a bucket and the key-0 node would miss an
observation) -- every planted read below puts such a window, or a near miss, where the two paths meet: at a lane's chunk boundary,
at a tile boundary, at a read boundary, in the ASCII form through N.

Shapes: k = 31 (every lane full) and k = 32 (the last lane of a read holds 14 windows), 150-base reads, 300 of them -- two whole
level-1 tiles of 128 reads and a partial one -- in the smallest table the PARTITION engine takes; the batch 2-bit packed without
offsets (regular tiles), as ASCII with offsets, and, a few reads trimmed to 60..149 bases, through the lane-prefix form.  Against
the oracle: sorted node dump, counts, and the key-0 node's link counters."""
import random

import numpy as np
import pytest

from helpers import set_hooks

READ_LEN, N_READS = 150, 300
KS = (31, 32)


def _background(rng):
    """300 random reads without a run of 16 equal bases"""
    reads = []
    while len(reads) < N_READS:
        r = "".join(rng.choice("ACGT") for _ in range(READ_LEN))
        if not any(b * 16 in r for b in "ACGT"):
            reads.append(r)
    return reads


def _plant(read, at, run):
    """`run` written over read[at:], the base on either side made a different one (the run is exactly that long)"""
    r = list(read)
    r[at:at + len(run)] = run
    assert len(r) == READ_LEN
    other = lambda b: "C" if b in "AN" else "G"
    if at > 0:
        r[at - 1] = other(run[0])
    if at + len(run) < READ_LEN:
        r[at + len(run)] = other(run[-1])
    return "".join(r)


# scenario -> (list of (read index, offset in the read, run), key 0 expected)
def _scenarios(k):
    first_aligned = lambda rd: (-(rd * READ_LEN)) % 16   # offset inside read rd of a 16-aligned flat position
    return {
        "none": ([], False),
        "k_A": ([(5, 40, "A" * k)], True),
        "k_minus_1_A_word_aligned": ([(7, first_aligned(7) + 16, "A" * (k - 1))], False),   # covers an all-A packed word, no window of k
        "k_T": ([(9, 77, "T" * k)], True),
        "k_N": ([(11, 3, "N" * k)], True),
        "run_from_window_14": ([(20, 14, "A" * k)], True),    # the key-0 window is the last one of lane 0 (15 windows per lane)
        "run_from_window_15": ([(21, 15, "T" * k)], True),    # ... the first one of lane 1
        "tile_boundary": ([(127, 100, "A" * k), (128, 0, "T" * k)], True),   # last read of a tile, first read of the next
        "across_reads": ([(30, READ_LEN - 20, "A" * 20), (31, 0, "A" * 20)], False),   # no window spans two reads
        "forty_A": ([(40, 50, "A" * 40)], True),               # 40 - k + 1 key-0 windows, over two lanes
    }


def _build_reads(k, name):
    rng = random.Random(1000 * k + len(name))
    reads = _background(rng)
    if name == "all":   # every planted read in one batch
        plants, expect = [p for pl, _ in _scenarios(k).values() for p in pl], True
    else:
        plants, expect = _scenarios(k)[name]
    for rd, at, run in plants:
        reads[rd] = _plant(reads[rd], at, run)
    return [r.encode() for r in reads], expect


def _key0_windows(reads, k):
    n = 0
    for r in reads:
        s = r.decode().upper().replace("N", "A")
        n += sum(1 for i in range(len(s) - k + 1) if s[i:i + k] in ("A" * k, "T" * k))
    return n


def _run_words(words):
    return int(np.count_nonzero((words == 0) | (words == 0xFFFFFFFF)))


def _check(g, st, ref, want, what):
    assert (st.total_reads, st.total_kmers, st.count) == (ref.total_reads, ref.total_kmers, ref.count), what
    assert np.array_equal(g.export_sorted(), want), what
    assert want[0]["kmer"] == 0   # (the key-0 node is always the dump's first row)
    assert (st.polyA_l_link, st.polyA_r_link) == (int(want[0]["l_link"]), int(want[0]["r_link"])), what


@pytest.fixture(scope="module")
def table_slots():
    from dbg_assembly_amd import capi
    return capi.find_next_prime_ref(1 << 26)   # the PARTITION engine needs 2^26 <= table_slots


NAMES = ["none", "k_A", "k_minus_1_A_word_aligned", "k_T", "k_N", "run_from_window_14", "run_from_window_15", "tile_boundary",
         "across_reads", "forty_A", "all"]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", NAMES)
def test_equal_length_forms_equal_oracle(oracle, table_slots, k, name):
    """regular tiles (2-bit packed, no offsets) and the same reads as ASCII"""
    from dbg_assembly_amd import capi
    reads, expect = _build_reads(k, name)
    bases, offsets = oracle.pack_reads(reads)
    words, other = capi.pack_bases(bases)
    assert other == 0
    n0 = _key0_windows(reads, k)
    assert (n0 > 0) == expect, (name, n0)
    if name == "none":
        assert _run_words(words) == 0          # no wave can see a word of sixteen A or T: all of them take the path without the test
    elif name == "k_minus_1_A_word_aligned":
        assert _run_words(words) >= 1 and n0 == 0   # the flag is raised, and there is no key 0
    elif name == "across_reads":
        assert n0 == 0
    ref = oracle.build_graph(files_mem=[(bases, offsets)], k=k, max_read_len=250, init_hash_size=0.001, threads=1)
    want = ref.nodes.astype(capi.NODE_DTYPE)
    key0_seen = bool(want[0]["l_link"]) or bool(want[0]["r_link"])
    assert key0_seen == expect, "the oracle's key-0 node and the planted reads disagree"
    for form in ("packed-uniform", "ascii"):
        with capi.Graph(k=k, table_slots=table_slots, max_read_len=250, engine=capi.ENGINE_PARTITION, expected_kmers=len(bases)) as g:
            if form == "ascii":
                g.push_reads(bases, offsets)
            else:
                g.push_reads_packed_uniform(words, N_READS, READ_LEN, other)
            st = g.finalize()
            _check(g, st, ref, want, (name, k, form))
            if not expect:
                assert (st.polyA_l_link, st.polyA_r_link) == (0, 0), (name, k, form)   # the key-0 node is empty


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", NAMES)
def test_prefix_form_equals_oracle(oracle, monkeypatch, table_slots, k, name):
    """the same reads, a few of the others trimmed to 60..149 bases: the lane-prefix form (reads of any lengths)"""
    from dbg_assembly_amd import capi
    reads, expect = _build_reads(k, name)
    planted = {rd for n, (pl, _) in _scenarios(k).items() for rd, _, _ in pl}
    rng = random.Random(77 + k)
    for rd in rng.sample([i for i in range(N_READS) if i not in planted and i + 1 not in planted], 25):
        reads[rd] = reads[rd][:rng.randint(60, 149)]
    assert (_key0_windows(reads, k) > 0) == expect
    bases, offsets = oracle.pack_reads(reads)
    words, other = capi.pack_bases(bases)
    ref = oracle.build_graph(files_mem=[(bases, offsets)], k=k, max_read_len=250, init_hash_size=0.001, threads=1)
    want = ref.nodes.astype(capi.NODE_DTYPE)
    set_hooks(monkeypatch, l1_prefix="1")
    for form in ("packed", "ascii"):
        with capi.Graph(k=k, table_slots=table_slots, max_read_len=250, engine=capi.ENGINE_PARTITION, expected_kmers=len(bases)) as g:
            if form == "ascii":
                g.push_reads(bases, offsets)
            else:
                g.push_reads_packed(words, offsets, other)
            st = g.finalize()
            assert g.timings().prefix_launches >= 1, "the batch did not take the prefix form"
            _check(g, st, ref, want, (name, k, form))
            if not expect:
                assert (st.polyA_l_link, st.polyA_r_link) == (0, 0), (name, k, form)
