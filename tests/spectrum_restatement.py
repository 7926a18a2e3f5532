"""The k-mer frequency spectrum restated in Python: write_kmer_spectrum of dbg_assembly_amd/host/kmer_spectrum.h (the
text of <lib>.kmer.freq.stat) and the numbers bin/kmerfreq feeds it.  tests/test_kmer_spectrum_cpu.py pins this
restatement to the reference's three files; the GPU tests then use it as what the tool must write."""
import numpy as np

COLUMNS = ("#Kmer_Frequency\tKmer_Species_Number\tKmer_Species_Ratio\tKmer_Species_accumulate_Ratio\tKmer_Individual_Number"
           "\tKmer_Individual_Ratio\tKmer_Individual_accumulate_ratio\n")


def _g(x):
    return "%g" % x   # an ostream's default formatting of a double


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def spectrum_text(k, max_freq, species, total_individuals):
    """species: {frequency: count} or a sequence indexed by frequency (entry 0 is not read)"""
    if isinstance(species, dict):
        sp = [0] * (max_freq + 1)
        for f, s in species.items():
            sp[f] = int(s)
    else:
        sp = [int(v) for v in species]
    total_species = sum(sp[1:max_freq + 1])
    out = ["#Kmer size: %d\n#Maximum Kmer frequency: %d\n#Kmer indivdual number: %d\n#Kmer species number: %d\n"
           "#Theoretic space of Kmer species: %d  occupied ratio: %s\n\n" % (k, max_freq, total_individuals, total_species, 4 ** k,
                                                                              _g(_ratio(total_species, 4 ** k))), COLUMNS]
    acc_s = acc_i = 0
    for f in range(1, max_freq + 1):
        ind = max(total_individuals - acc_i, 0) if f == max_freq else f * sp[f]
        acc_s += sp[f]
        acc_i += ind
        out.append("%d\t%d\t%s\t%s\t%d\t%s\t%s\n" % (f, sp[f], _g(_ratio(sp[f], total_species)), _g(_ratio(acc_s, total_species)), ind,
                                                     _g(_ratio(ind, total_individuals)), _g(_ratio(acc_i, total_individuals))))
    return "".join(out)


def canonical_counts(reads, k):
    """{canonical k-mer value: occurrences} over every window of every read, as the KFREQ engine counts: ACGT = 0..3 in
    either case, N and any other byte = A, canonical = min(forward, reverse complement)"""
    code = np.zeros(256, dtype=np.int64)
    for ch, v in zip(b"CGTcgt", (1, 2, 3, 1, 2, 3)):
        code[ch] = v
    counts = {}
    mask = 4 ** k - 1
    for r in reads:
        c = code[np.frombuffer(bytes(r), dtype=np.uint8)]
        if len(c) < k:
            continue
        fw = rc = 0
        for i, b in enumerate(c):
            b = int(b)
            fw = ((fw << 2) | b) & mask
            rc = (rc >> 2) | ((3 - b) << (2 * (k - 1)))
            if i >= k - 1:
                v = min(fw, rc)
                counts[v] = counts.get(v, 0) + 1
    return counts
