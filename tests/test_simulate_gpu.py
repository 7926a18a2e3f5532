"""GPU: simulate_lowfreq_kmer -- Corrector.mutation_scan (k_mut_scan) returns the bins of the Python restatement
(tests/simulate_restatement.py, pinned to the real program by tests/test_simulate_cpu.py) on every golden genome and at
the site counts, skips and k-mer sizes where the kernel's own structure could go wrong, and bin/simulate_lowfreq_kmer
prints every golden byte for byte."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simulate_restatement as SIM  # noqa: E402

EXE = os.path.join(ROOT, "dbg_assembly_amd", "bin", "simulate_lowfreq_kmer")
GOLDEN = os.path.join(ROOT, "tests", "golden", "simulate_cases")
CASES = json.load(open(os.path.join(GOLDEN, "cases.json")))
pytestmark = pytest.mark.gpu


def options_of(case):
    o = dict(zip(case["args"][0::2], case["args"][1::2]))
    return int(o.get("-k", 17)), int(o.get("-s", 100))


def rand_seq(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def partial_fragments(g, k, skip, n):
    """for the first n sites of g: the mutated fragment of 2k - 1 bases without its first m % k bases -- a record too short to
    have a site of its own whose windows are the last k - m % k windows of that site: every bin of the scan fills"""
    out = []
    for m in range(n):
        i = m * skip
        frag = bytearray(g[i:i + 2 * k - 1])
        frag[k - 1] = b"ACGT"[(b"ACGT".index(bytes([frag[k - 1]]).upper()) + 1) % 4]
        out.append(bytes(frag[m % k:]))
    return out


class Table:
    """the genome's k-mers on both strands, as the program builds them: a KFREQ handle, then the corrector's bit table"""

    def __init__(self, seqs, k):
        from dbg_assembly_amd import capi
        self.capi = capi
        with capi.Graph(k=k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000000) as g:
            g.push_reads(*capi.concat_sequences(seqs))
            g.finalize()
            self.c = capi.Corrector(k=k)
            self.c.from_kfreq(g, 0)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.c.close()

    def scan(self, seqs, skip):
        return self.c.mutation_scan(*self.capi.concat_sequences(seqs), skip)


def expected_hist(seqs, k, skip):
    return SIM.mutation_scan(seqs, k, skip, SIM.lookup_in_values(SIM.table_of(seqs, k))).astype(np.uint64)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_mutation_scan_equals_restatement_on_golden_genome(case):
    k, skip = options_of(case)
    seqs = SIM.read_genome(os.path.join(GOLDEN, case["file"]))
    with Table(seqs, k) as t:
        got = t.scan(seqs, skip)
        assert got.shape == (k + 1,) and np.array_equal(got, expected_hist(seqs, k, skip))
        assert t.c.mutation_scan_ms() > 0 and t.c.batch_stats()["reads"] == 0   # timed apart; the batch statistics are left alone


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_program_prints_the_golden_stdout(case):
    r = subprocess.run([EXE] + case["args"] + [os.path.join(GOLDEN, case["file"])], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout == open(os.path.join(GOLDEN, case["name"] + ".stdout"), "rb").read()


@pytest.mark.parametrize("sites", [63, 64, 65, 255, 256, 257])
def test_site_counts_around_a_wave_and_a_workgroup_restatement_only(sites):
    k, skip = 9, 3
    rng = random.Random(sites)
    one = rand_seq(rng, 2 * k - 1 + (sites - 1) * skip, b"AC")   # two letters: a mutated window is often another window of it
    assert SIM.site_count(len(one), k, skip) == sites
    with Table([one], k) as t:
        want = expected_hist([one], k, skip)
        assert int(want.sum()) == sites and np.count_nonzero(want) >= 3
        assert np.array_equal(t.scan([one], skip), want)
        # the same sites spread over records, with records that have no site (empty, shorter than k, 2k - 2 bases) between them
        cut = [one[:17], b"", one[:30], one[:5], one[:16], one, rand_seq(rng, 16), one[:2 * k - 1 + skip], b"ACGT"]
        with Table(cut, k) as t2:
            want = expected_hist(cut, k, skip)
            assert int(want.sum()) == 1 + 5 + sites + 2
            assert np.array_equal(t2.scan(cut, skip), want)


def test_skip_1_and_argument_checks():
    k = 11
    rng = random.Random(1)
    g = rand_seq(rng, 3000)
    seqs = [g, g[100:900] + rand_seq(rng, 50) + g[1000:1500], b"N" * 40 + g[:60].lower()]
    with Table(seqs, k) as t:
        for skip in (1, 2, 1 << 31):
            want = expected_hist(seqs, k, skip)
            assert np.array_equal(t.scan(seqs, skip), want)
        assert np.count_nonzero(expected_hist(seqs, k, 1)) >= 4
        assert int(t.scan([], 5).sum()) == 0 and int(t.scan([b"ACGT"], 5).sum()) == 0   # no sequence / no site
        with pytest.raises(t.capi.DbgkError) as e:
            t.scan(seqs, 0)
        assert e.value.status == t.capi.ERR_ARG
        bases, offsets = t.capi.concat_sequences(seqs)
        for bad_offsets, bad_skip in ((offsets[:0], 5), (offsets, 1 << 32), (offsets, -1), (np.append(offsets, offsets[-1] + 1), 5)):
            with pytest.raises(ValueError):   # refused by the wrapper: no sequence count of 2^64 - 1, no skip cut to 32 bits
                t.c.mutation_scan(bases, bad_offsets, bad_skip)
    from dbg_assembly_amd import capi
    with capi.Corrector(k=k) as c:   # no table yet
        with pytest.raises(capi.DbgkError) as e:
            c.mutation_scan(*capi.concat_sequences(seqs), 5)
        assert e.value.status == capi.ERR_STATE


@pytest.mark.parametrize("k", [16, 18])
def test_large_k_on_a_short_genome_restatement_only(k):
    rng = random.Random(k)
    g = rand_seq(rng, 1500)
    seqs = [g, g[200:700].lower()] + partial_fragments(g, k, 50, 25)
    with Table(seqs, k) as t:
        for skip in (1, 50):
            want = expected_hist(seqs, k, skip)
            assert np.array_equal(t.scan(seqs, skip), want)
        assert np.count_nonzero(expected_hist(seqs, k, 50)) == k + 1


@pytest.mark.parametrize("k", [4, 6, 16])
def test_species_number_with_kmers_that_are_their_own_reverse_complement_restatement_only(tmp_path, k):
    """even k: such a k-mer is one set bit of the table, every other canonical k-mer two"""
    rng = random.Random(100 + k)
    pal = [b"ACGT" * (k // 4) + b"AT" * (k % 4 // 2), b"A" * (k // 2) + b"T" * (k // 2), b"T" * (k // 2) + b"A" * (k // 2)]
    seqs = [rand_seq(rng, 300) + pal[0] + rand_seq(rng, 40) + pal[1] + pal[0], pal[2] + rand_seq(rng, 2 * k), b"T" * (2 * k)]
    table = SIM.table_of(seqs, k)
    assert np.count_nonzero(SIM.revcomp_values(table, k) == table) >= 3
    fa = tmp_path / "g.fa"
    fa.write_bytes(b"".join(b">s\n" + s + b"\n" for s in seqs))
    r = subprocess.run([EXE, "-k", str(k), "-s", "3", str(fa)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.decode() == SIM.report(seqs, k, 3)


def test_defaults_k17_lookups_on_the_exported_bits_and_the_program(tmp_path):
    """k = 17, -s 100 (no options): the scan against the restatement's lookups done on the 2 GiB of bits the device holds, and
    the program's stdout against the whole restatement"""
    k, skip = 17, 100
    rng = random.Random(17)
    g = rand_seq(rng, 20000)
    seqs = [g, g[12000:15000].lower() + b"NN" + g[100:2000], b"T" * 400] + partial_fragments(g, k, skip, 60)
    with Table(seqs, k) as t:
        got = t.scan(seqs, skip)
        bits = t.c.export_bits()
        assert bits.size == 4 ** k // 8
        want = SIM.mutation_scan(seqs, k, skip, SIM.lookup_in_bits(bits)).astype(np.uint64)
        assert np.array_equal(got, want) and np.count_nonzero(got) >= 3
        assert np.array_equal(want, expected_hist(seqs, k, skip))
        species = int(np.bitwise_count(bits).sum()) - int(bits[-1] & 1)
    fa = tmp_path / "genome.fa"
    fa.write_bytes(b"junk\n" + b"".join(b">s%d x\n" % i + b"\n".join(s[p:p + 70] for p in range(0, len(s), 70)) + b"\n" for i, s in enumerate(seqs)))
    r = subprocess.run([EXE, str(fa)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.decode() == SIM.report(seqs, k, skip)
    assert r.stdout.decode() == SIM.report(seqs, k, skip, hist=got, species=species)
