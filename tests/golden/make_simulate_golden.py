"""Generate the simulate_lowfreq_kmer golden vectors with the REAL reference program: tests/golden/simulate_cases/ holds,
per case, the genome file, and in cases.json its name, file and arguments; <case>.stdout is what the reference printed,
simulate_usage.txt its usage text.  The fixtures are data; this script needs the reference only when it is run.

The binary is compiled here by the reference Makefile's rule (correct_error/Makefile:16-17):

    g++ -O3 -o simulate_lowfreq_kmer simulate_lowfreq_kmer.cpp seqKmer.cpp gzstream.cpp -lz

    python tests/golden/make_simulate_golden.py /path/to/reference/correct_error

No record is shorter than 2k - 1 bases (the reference aborts on those) and no byte is outside ACGTNacgtn.
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "simulate_cases")


def rand_seq(rng, n, letters="ACGT"):
    return "".join(rng.choice(list(letters), size=n))


def de_bruijn(k):
    """every k-mer over ACGT once (cyclic), opened up: 4^k + k - 1 bases"""
    a = [0] * (4 * k)
    seq = []

    def db(t, p):
        if t > k:
            if k % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = "".join("ACGT"[i] for i in seq)
    return s + s[:k - 1]


def fasta(records, width=60):
    out = []
    for i, s in enumerate(records):
        out.append(">chr%d some description\n" % (i + 1))
        out.extend(s[p:p + width] + "\n" for p in range(0, len(s), width))
    return "".join(out)


def messy(rng, records):
    """lines of varying width, lower case, N, spaces inside lines, an empty line, text before the first header"""
    out = ["text before the first header is ignored\n\n"]
    for i, s in enumerate(records):
        s = list(s)
        for p in range(len(s)):
            u = rng.random()
            if u < 0.01:
                s[p] = "N"
            elif u < 0.02:
                s[p] = "n"
            elif u < 0.3:
                s[p] = s[p].lower()
        s = "".join(s)
        out.append(">rec%d\n" % i)
        p = 0
        while p < len(s):
            w = int(rng.integers(1, 90))
            line = s[p:p + w]
            if len(line) > 4 and rng.random() < 0.3:
                cut = int(rng.integers(1, len(line)))
                line = line[:cut] + " " + line[cut:]
            out.append(line + "\n")
            if rng.random() < 0.05:
                out.append("\n")
            p += w
    return "".join(out)


def cases():
    rng = np.random.default_rng(20261019)
    k9s7_exact = 17 + 7 * 30          # the last site starts exactly at L - (2k - 1)
    out = [
        # name, file, text, gz, arguments
        ("k1_s1", "k1.fa", fasta([rand_seq(rng, 300)]), False, ["-k", "1", "-s", "1"]),
        ("k2_s7", "k2.fa", fasta([rand_seq(rng, 500), rand_seq(rng, 41)]), False, ["-k", "2", "-s", "7"]),
        ("k5_every_kmer", "k5_debruijn.fa", fasta([de_bruijn(5)]), False, ["-k", "5", "-s", "7"]),
        ("k9_messy_default_skip", "k9_messy.fa", messy(rng, [rand_seq(rng, 2500), rand_seq(rng, 17), rand_seq(rng, 900)]), False, ["-k", "9"]),
        ("k9_messy_s1", "k9_messy.fa", None, False, ["-k", "9", "-s", "1"]),
        ("k9_exactly_2k_minus_1", "k9_17bases.fa", fasta([rand_seq(rng, 17)]), False, ["-k", "9", "-s", "3"]),
        ("k9_last_site_at_the_end", "k9_exact.fa", fasta([rand_seq(rng, k9s7_exact)], 70), False, ["-k", "9", "-s", "7"]),
        ("k9_one_base_short", "k9_short.fa", fasta([rand_seq(rng, k9s7_exact - 1)], 70), False, ["-k", "9", "-s", "7"]),
        ("k9_skip_beyond_sequence", "k9_exact.fa", None, False, ["-k", "9", "-s", "100000"]),
        ("k9_polyA", "k9_polyA.fa", fasta(["A" * 200]), False, ["-k", "9", "-s", "7"]),
        ("k9_two_letters", "k9_AC.fa", fasta([rand_seq(rng, 700, "AC"), rand_seq(rng, 300, "AC")]), False, ["-k", "9", "-s", "2"]),
        ("k5_period3", "k5_period3.fa", fasta(["ACG" * 120 + rand_seq(rng, 60) + "ACG" * 40]), False, ["-k", "5", "-s", "1"]),
        ("k13_gz", "k13.fa.gz", fasta([rand_seq(rng, 3000), rand_seq(rng, 2000).lower()], 80), True, ["-k", "13", "-s", "5"]),
        ("k16_s50", "k16.fa", fasta([rand_seq(rng, 3000)]), False, ["-k", "16", "-s", "50"]),
    ]
    return out


def main():
    src = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "simulate_lowfreq_kmer")
        subprocess.run(["g++", "-O3", "-o", exe, "simulate_lowfreq_kmer.cpp", "seqKmer.cpp", "gzstream.cpp", "-lz"], cwd=src, check=True)
        open(os.path.join(OUT, "simulate_usage.txt"), "wb").write(subprocess.run([exe, "-h"], capture_output=True, timeout=60).stdout)
        meta = []
        for name, fname, text, gz, args in cases():
            path = os.path.join(OUT, fname)
            if text is not None:
                with open(path, "wb") as f:
                    if gz:
                        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:   # no time stamp: a rerun writes the same bytes
                            z.write(text.encode())
                    else:
                        f.write(text.encode())
            r = subprocess.run([exe] + args + [path], capture_output=True, timeout=600)
            assert r.returncode == 0, (name, r.returncode, r.stderr[-500:])
            open(os.path.join(OUT, name + ".stdout"), "wb").write(r.stdout)
            meta.append({"name": name, "file": fname, "args": args})
            print(name, r.stdout.decode().split("\n")[2], "|", r.stdout.decode().split("\n")[7])
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(m) for m in meta) + "\n]\n")


if __name__ == "__main__":
    main()
