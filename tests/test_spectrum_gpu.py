"""GPU: the k-mer frequency spectrum binned on the device (k_kf_spectrum, dbgk_kfreq_spectrum / dbgk_comm_kfreq_spectrum)
equals np.bincount of the exported counters for every table shape and range, and `kmerfreq` writes the
<prefix>.kmer.freq.stat that the (reference-pinned) restatement of the writer gives for those bins."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spectrum_restatement as SR  # noqa: E402

TOOL = os.path.join(ROOT, "dbg_assembly_amd", "bin", "kmerfreq")
pytestmark = pytest.mark.gpu


def pack(reads):
    from dbg_assembly_amd import capi
    return capi.concat_sequences(reads)


def random_reads(seed, n, length, letters=b"ACGT"):
    rng = random.Random(seed)
    return [bytes(rng.choice(letters) for _ in range(length)) for _ in range(n)]


def genome_reads(seed, n, genome_len=4000, length=100):
    """reads off a small genome, a tenth of them repeated: counters from 1 up to saturation"""
    rng = random.Random(seed)
    g = bytes(rng.choice(b"ACGT") for _ in range(genome_len))
    out = [g[s:s + length] for s in (rng.randint(0, genome_len - length) for _ in range(n))]
    return out + [b"A" * 90] * 300 + [b"ACGTTGCA" * 12] * 20 + [b"acgtn" * 20, b"", b"ACG"]


def counted(k, reads, expected=0):
    from dbg_assembly_amd import capi
    g = capi.Graph(k=k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000000, expected_kmers=expected)
    g.push_reads(*pack(reads))
    g.finalize()
    return g


def check(g, first=0, n=None):
    n = 4 ** g.k - first if n is None else n
    got = g.kfreq_spectrum(first, n)
    want = np.bincount(g.kfreq_counts(first, n), minlength=256).astype(np.uint64)
    assert got.dtype == np.uint64 and got.shape == (256,)
    assert np.array_equal(got, want), (first, n, np.flatnonzero(got != want)[:8])
    assert int(got.sum()) == n
    return got


def test_k4_every_counter_saturated_all_lanes_hit_one_bin():
    with counted(4, random_reads(4, 2000, 100)) as g:
        got = check(g)
        assert got[255] == 136 and got[0] == 120   # the 136 canonical 4-mers at 255, their 120 mirror values never counted
        assert g.kfreq_spectrum_ms() > 0
        g.kfreq_spectrum(7, 0)
        assert g.kfreq_spectrum_ms() == 0   # no kernel ran


def test_k6_dense():
    with counted(6, random_reads(6, 300, 100)) as g:
        got = check(g)
        assert np.count_nonzero(got[1:]) > 15 and got[0] < 4 ** 6 // 2 + 100


@pytest.mark.parametrize("k", [8, 9])
def test_small_tables(k):
    with counted(k, genome_reads(k, 1500)) as g:
        got = check(g)
        assert got[255] >= 1 and np.count_nonzero(got[1:]) > 10


@pytest.mark.parametrize("expected", [0, 400000], ids=["atomics", "direct_blocks"])
def test_k13_64MiB_nearly_all_zero(expected):
    with counted(13, genome_reads(13, 3000), expected) as g:
        got = check(g)
        assert got[0] > 4 ** 13 - 10000
        check(g, 4 ** 13 // 3 + 5, 4 ** 13 // 2 + 7)


def test_254_255_256_occurrences_and_the_remainder_rule():
    k = 9
    kmers = [b"ACGTACGGA", b"CCGTTAGCA", b"GATTACAGA"]
    reads = [kmers[0]] * 254 + [kmers[1]] * 255 + [kmers[2]] * 256
    with counted(k, reads) as g:
        got = check(g)
        assert (got[254], got[255], int(got[1:].sum())) == (1, 2, 3)
        rows = SR.spectrum_text(k, 255, got, len(reads)).split("\n")
        # row 255 is "255 or more": its individuals are what the rows before leave of the 765 windows, the columns end at 1
        assert rows[7 + 253] == "254\t1\t0.333333\t0.333333\t254\t0.332026\t0.332026"
        assert rows[7 + 254] == "255\t2\t0.666667\t1\t511\t0.667974\t1"


def test_ranges_heads_tails_and_errors():
    from dbg_assembly_amd import capi
    k = 9
    total = 4 ** k
    with counted(k, random_reads(9, 2500, 100)) as g:   # 230 k windows over 131 k canonical values: few quads are zero
        assert np.count_nonzero(g.kfreq_counts(0, 4096)) > 1000
        for first in (0, 16, 5, 1000 * 16 + 15):
            for n in (0, 1, 15, 16, 17):
                check(g, first, n)
        check(g, 35, 5)                   # inside one 16-byte quad
        check(g, 33, 14)                  # inside one quad, up to its last byte but one
        check(g, 5, 16 * 40 - 5)          # misaligned first, aligned end
        check(g, 16 * 7, 16 * 40 + 9)     # aligned first, misaligned end
        check(g, 7, 16 * 1000 + 1)        # both misaligned, many quads
        check(g, total - 16 * 3 - 3, 16 * 3 + 3)   # ends at 4^k
        check(g, total - 1, 1)
        check(g, total, 0)
        for first, n in ((total, 1), (0, total + 1), (total + 1, 0), (5, total)):
            with pytest.raises(capi.DbgkError) as e:
                g.kfreq_spectrum(first, n)
            assert e.value.status == capi.ERR_ARG
    with capi.Graph(k=k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000) as g:
        g.push_reads(*pack([b"ACGTACGTACGT"]))
        with pytest.raises(capi.DbgkError) as e:   # not finalized
            g.kfreq_spectrum()
        assert e.value.status == capi.ERR_STATE


def test_k17_indices_beyond_2_pow_32():
    """A 17-mer that begins with T and ends with A has a reverse complement that does too: both values, so the canonical
    one, lie above 3 * 2^32.  Eight more k-mers sit right around 2^32, each pushed a different number of times."""
    k = 17
    rng = random.Random(17)
    reads = [b"T" + bytes(rng.choice(b"ACGT") for _ in range(15)) + b"A" for _ in range(5000)]
    reads += reads[:300] + reads[:40] * 3
    near = [b"A" + b"T" * 15 + b"G", b"A" + b"T" * 15 + b"C", b"A" + b"T" * 15 + b"A", b"C" + b"A" * 16, b"C" + b"A" * 15 + b"C",
            b"C" + b"A" * 15 + b"G", b"C" + b"A" * 14 + b"CA", b"A" + b"T" * 14 + b"GC"]
    for i, km in enumerate(near):
        reads += [km] * (i + 2)
    truth = SR.canonical_counts(reads, k)
    assert min(v for v in truth if v >= 3 << 32) > 1 << 33 and sum(1 for v in truth if v >= 3 << 32) >= 4990
    assert sorted(v - (1 << 32) for v in truth if v < 3 << 32) == [-7, -4, -3, -2, 0, 1, 2, 4]
    want = np.bincount(np.minimum(np.array(list(truth.values())), 255), minlength=256).astype(np.uint64)
    want[0] = 4 ** k - len(truth)
    with counted(k, reads) as g:
        got = check(g, (1 << 32) - 24, 48)
        assert int(got[1:].sum()) == 8 and int(got[2:10].sum()) == 8
        assert np.array_equal(g.kfreq_spectrum(), want)          # the whole 16 GiB table, against the k-mers counted on the host
        got = check(g, (3 << 32) - 5, (1 << 28) + 11)            # 256 MiB above 2^33 against the exported counters
        assert int(got[1:].sum()) > 200


def test_communicator_of_three_members_equals_one_handle():
    from dbg_assembly_amd import capi
    k = 12
    reads = genome_reads(12, 4000)
    with counted(k, reads) as g:
        want = check(g)
    with capi.Comm(k, 0, [0] * 3, max_read_len=1000000, expected_kmers=150000, engine=capi.ENGINE_KFREQ) as c:
        for i in range(0, len(reads), 450):
            c.push_reads(*pack(reads[i:i + 450]))
        with pytest.raises(capi.DbgkError):   # not finalized
            c.kfreq_spectrum()
        c.finalize()
        got = c.kfreq_spectrum()
        assert np.array_equal(got, want) and int(got.sum()) == 4 ** k
        assert np.array_equal(got, np.bincount(c.kfreq_counts(), minlength=256).astype(np.uint64))


@pytest.mark.parametrize("bits,env", [(1, {}), (8, {}), (8, {"DBGK_GPU_LIST": "0,0,0", "DBGK_BATCH_BYTES": "30000"})],
                         ids=["b1", "b8", "b8_three_members"])
def test_kmerfreq_tool_writes_the_spectrum_file(tmp_path, bits, env):
    k = 9
    reads = [r for r in genome_reads(99, 1200) if r]
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">r\n" + r + b"\n" for r in reads))
    lib = tmp_path / "reads.lib"
    lib.write_text(str(fa) + "\n")
    prefix = str(tmp_path / "out")
    r = subprocess.run([TOOL, "-k", str(k), "-f", "2", "-b", str(bits), "-t", "2", "-o", prefix, str(lib)], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stderr.strip().splitlines()[-1].startswith("wrote ")   # the stderr lines are the ones the tool had
    truth = SR.canonical_counts(reads, k)
    windows = sum(max(0, len(x) - k + 1) for x in reads)
    assert sum(truth.values()) == windows
    bins = np.bincount(np.minimum(np.array(list(truth.values())), 255), minlength=256)
    text = open(prefix + ".kmer.freq.stat").read()
    assert text == SR.spectrum_text(k, 255, bins, windows)
    head = text.split("\n")
    assert head[2] == "#Kmer indivdual number: %d" % windows and head[3] == "#Kmer species number: %d" % len(truth)
    assert len(head) == 7 + 255 + 1 and head[-2].split("\t")[3] == "1" and head[-2].split("\t")[6] == "1"
    assert os.path.exists(prefix + ".kmer.freq.cz") and os.path.exists(prefix + ".kmer.freq.cz.len")
