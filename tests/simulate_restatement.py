"""simulate_lowfreq_kmer (correct_error/simulate_lowfreq_kmer.cpp) restated in Python: the reader, the k-mer table on
both strands, the mutation scan and the printing.  tests/test_simulate_cpu.py pins it to what the real program wrote
(tests/golden/simulate_cases); the GPU tests then use it where no golden exists.

Outside what it restates: a record shorter than 2k - 1 bases (the reference aborts; here it simply has no site) and bytes
outside ACGTNacgtn (the reference reads past its alphabet table; here they are A)."""
import gzip

import numpy as np

CODE = np.zeros(256, dtype=np.int64)   # A = a = N = n = 0 (seqKmer.cpp:10), and so is every other byte
for _ch, _v in zip(b"CGTcgt", (1, 2, 3, 1, 2, 3)):
    CODE[_ch] = _v


def read_genome(path):
    """-> list of bytes: text before the first '>' is ignored; a record is a header line, then everything up to the next
    '>' with newlines and spaces removed"""
    raw = open(path, "rb").read()
    text = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
    seqs = []
    at = text.find(b">")
    while at != -1 and at + 1 < len(text):
        eol = text.find(b"\n", at + 1)
        if eol == -1:
            break
        nxt = text.find(b">", eol + 1)
        body = text[eol + 1:len(text) if nxt == -1 else nxt]
        seqs.append(body.replace(b"\n", b"").replace(b" ", b""))
        at = nxt
    return seqs


def window_values(seq, k):
    """forward value of every k-mer window of seq (seq2bit), int64[len - k + 1]"""
    c = CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    v = np.zeros(n, dtype=np.int64)
    for t in range(k):
        v = v * 4 + c[t:t + n]
    return v


def revcomp_values(v, k):
    out = np.zeros_like(v)
    w = v.copy()
    for _ in range(k):
        out = out * 4 + (3 - (w & 3))
        w >>= 2
    return out


def table_of(seqs, k):
    """the sorted values of every k-mer of either strand"""
    parts = [window_values(s, k) for s in seqs]
    fw = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return np.unique(np.concatenate([fw, revcomp_values(fw, k)]))


def lookup_in_values(table):
    return lambda v: np.isin(v, table)


def lookup_in_bits(bits):
    """bits: the exported 1-bit table, bit v = bit 128 >> v % 8 of byte v / 8"""
    return lambda v: (bits[v >> 3] & (np.uint8(128) >> (v & 7).astype(np.uint8))) != 0


def site_count(length, k, skip):
    return (length - (2 * k - 1)) // skip + 1 if length >= 2 * k - 1 else 0


def mutation_scan(seqs, k, skip, lookup):
    """-> int64[k + 1]: hist[j] = sites with j of the k windows over the mutated base absent from the table"""
    hist = np.zeros(k + 1, dtype=np.int64)
    for s in seqs:
        n = site_count(len(s), k, skip)
        if n == 0:
            continue
        c = CODE[np.frombuffer(bytes(s), dtype=np.uint8)]
        vals = window_values(s, k)
        start = np.arange(n, dtype=np.int64) * skip
        old = c[start + k - 1]
        delta = ((old + 1) & 3) - old
        absent = np.zeros(n, dtype=np.int64)
        for j in range(k):   # window j starts at start + j; the mutated base is its base k - 1 - j, of weight 4^j
            absent += ~lookup(vals[start + j] + delta * 4 ** j)
        hist += np.bincount(absent, minlength=k + 1)
    return hist


def _g(x):
    return "%g" % x


def report(seqs, k, skip, hist=None, species=None):
    """the program's stdout.  hist / species: taken from elsewhere (a device run) instead of being computed here"""
    table = None
    if species is None or hist is None:
        table = table_of(seqs, k)
    if species is None:
        species = len(table) - int(len(table) > 0 and table[-1] == 4 ** k - 1)   # the loop stops before the all-T k-mer
    if hist is None:
        hist = mutation_scan(seqs, k, skip, lookup_in_values(table))
    hist = [int(v) for v in hist]
    genome = sum(len(s) for s in seqs)
    total = sum(len(s) - k + 1 for s in seqs)
    out = "The Genome size is:  %d\nKmer total number:   %d\nKmer species number: %d\n\n" % (genome, total, species)
    groups = sum(hist)
    if groups == 0:
        raise ValueError("no mutation site: the ratios are 0 / 0")
    low = sum(i * hist[i] for i in range(k + 1))
    at_least = lambda r: sum(hist[i] for i in range(k + 1) if i / k >= r)  # noqa: E731
    out += "\nKmer size: %d\n" % k
    out += "\nRatio of low-freq kmers in all kmers by muation : %s\n" % _g(low / (groups * k))
    out += "\nRatio of mutations with 100%% low-freq kmers:  %s\n" % _g(hist[k] / groups)
    out += "\nRatio of mutations with >=80%% low-freq kmers: %s\n" % _g(at_least(0.8) / groups)
    out += "\nRatio of mutations with >=50%% low-freq kmers: %s\n" % _g(at_least(0.5) / groups)
    out += "\nRatio of mutations with >=20%% low-freq kmers: %s\n" % _g(at_least(0.2) / groups)
    out += "\nRatio of mutations with >= 1 low-freq kmers:  %s\n" % _g(sum(hist[1:]) / groups)
    return out
