"""Writes tests/golden/clean_cases: small inputs, and what the REFERENCE's own clean_adapter and clean_lowqual make of them.

    python tests/golden/make_clean_golden.py <directory of the reference>

The two programs are taken ready built from <reference>/clean_illumina/ (they need libz and libstdc++ only).  Nothing of the
reference but data is stored: its three adapter FASTA files, the usage texts its programs print and their output files.  No test
runs this script; the tests read what it left.  The inputs are made so that every category the tests ask for occurs, which the
script checks with tests/clean_restatement.py before it stores anything.
"""
import gzip
import json
import os
import random
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clean_restatement as CR  # noqa: E402

OUT = os.path.join(HERE, "clean_cases")
ADAPTER_FILES = ("illumina_NEB_adapter.fa", "illumina_NEB_adapter_R1.fa", "illumina_NEB_adapter_R2.fa")


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def other_base(c):
    return "ACGT"[("ACGT".index(c.upper()) + 1) % 4] if c.upper() in "ACGT" else "A"


def qualities(rng, n, shift, kind):
    """kind 0: high throughout, 1: a low tail, 2: low throughout, 3: a low stretch in the middle"""
    hi, lo = [40, 40, 41, 37, 41], [2, 2, 12, 20, 30, 8]
    q = []
    for j in range(n):
        low = (kind == 1 and j > n * 0.6) or kind == 2 or (kind == 3 and n * 0.4 < j < n * 0.5)
        q.append(chr(shift + rng.choice(lo if low and rng.random() < 0.8 else hi)))
    return "".join(q)


def adapter_reads(rng, adapters, cutoff, tag):
    """reads for one adapter set: hits, no hit, adapter near the front, two cells tying for the maximum, a later adapter that scores
    higher than the first one that reaches the cutoff"""
    reads = []
    first = adapters[0][1]
    later = max(adapters[1:], key=lambda a: len(a[1]))[1] if len(adapters) > 1 else first
    for n, (_, ad) in enumerate(adapters):
        piece = ad[:min(len(ad), 24)]
        reads.append(("%s_hit%d" % (tag, n), rand_seq(rng, 110 + 7 * n) + piece + rand_seq(rng, 5)))
        reads.append(("%s_tail%d" % (tag, n), rand_seq(rng, 130) + piece[:max(cutoff + 2, 9)]))
    reads.append((tag + "_front", rand_seq(rng, 12) + first[:30] + rand_seq(rng, 90)))
    for n in range(4):
        reads.append(("%s_none%d" % (tag, n), rand_seq(rng, rng.choice([76, 100, 150, 151]))))
    m = min(len(first), cutoff + 3)
    tie = rand_seq(rng, 80) + first[:m] + other_base(first[m % len(first)]) + other_base(first[0]) + first[:m] + other_base(first[m % len(first)])
    reads.append((tag + "_tie", tie + rand_seq(rng, 3)))
    k = min(len(first), cutoff + 1)
    reads.append((tag + "_later", rand_seq(rng, 90) + first[:k] + other_base(first[k % len(first)]) + rand_seq(rng, 6) + later[:30]))
    mutated = "".join(rng.choice("ACGT") if rng.random() < 0.08 else c for c in first)
    reads.append((tag + "_mut", rand_seq(rng, 100) + mutated))
    return reads


def fastq(rng, reads, shift, junk=False):
    lines = []
    for n, (name, seq) in enumerate(reads):
        qual = qualities(rng, len(seq), shift, n % 4)
        if name.endswith("_shortqual"):
            qual = qual[:-3]
        if junk and n % 5 == 2:
            lines += ["this line belongs to no record", ""]
        lines += ["@%s/1 extra" % name, seq, "+", qual]
    return "\n".join(lines) + "\n"


def main():
    ref = os.path.join(sys.argv[1], "clean_illumina")
    rng = random.Random(20261016)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    for f in ADAPTER_FILES:
        shutil.copy(os.path.join(ref, f), os.path.join(OUT, f))
    neb = CR.read_fasta(open(os.path.join(OUT, ADAPTER_FILES[0])).read(), 0)

    # a contaminant file of our own: 130 bases over several lines with one N, and 8 bases
    long_c = rand_seq(rng, 130)
    long_c = long_c[:57] + "N" + long_c[58:]
    short_c = "GTCCATGA"
    with open(os.path.join(OUT, "contaminants.fa"), "w") as f:
        f.write(">long130 a description\n%s\n%s\n%s\n>short8\tanother\n%s\n" % (long_c[:50], long_c[50:100], long_c[100:], short_c))
    contam = CR.read_fasta(open(os.path.join(OUT, "contaminants.fa")).read(), 1)

    plain = adapter_reads(rng, neb, 12, "neb")
    open(os.path.join(OUT, "reads.fq"), "w").write(fastq(rng, plain, 33))

    mixed = adapter_reads(rng, neb, 12, "neb") + adapter_reads(rng, contam, 8, "con")
    mixed += [("len30", rand_seq(rng, 30)), ("len600", rand_seq(rng, 600)), ("len1500", rand_seq(rng, 1480) + neb[1][1][:20]),
              ("len2000", rand_seq(rng, 1200) + CR.reverse_complement(long_c)[:60] + rand_seq(rng, 740)),
              ("lower", (rand_seq(rng, 100) + neb[0][1]).lower()), ("empty", ""), ("len100_shortqual", rand_seq(rng, 100)),
              ("allN", "N" * 80)]
    mixed += [("withN%d" % n, "".join("N" if rng.random() < 0.05 else c for c in rand_seq(rng, 120) + neb[n % 2][1][:18])) for n in range(3)]
    rng.shuffle(mixed)
    text = fastq(rng, mixed, 33, junk=True)
    open(os.path.join(OUT, "mixed.fq"), "w").write(text)
    with gzip.GzipFile(os.path.join(OUT, "mixed.fq.gz"), "wb", mtime=0) as f:
        f.write(text.encode())
    open(os.path.join(OUT, "phred64.fq"), "w").write(fastq(rng, plain[:16] + [("q64_N", "ACGTN" * 20)], 64))
    open(os.path.join(OUT, "norecords.fq"), "w").write("no record in this file\n\n+\n")

    cases = [
        {"name": "adapter_default", "program": "clean_adapter", "args": ["-a", "illumina_NEB_adapter.fa"], "input": "reads.fq"},
        {"name": "adapter_contaminants", "program": "clean_adapter", "args": ["-a", "contaminants.fa", "-b", "1", "-s", "8", "-r", "40"],
         "input": "mixed.fq.gz"},
        {"name": "adapter_mixed_plain", "program": "clean_adapter", "args": ["-a", "illumina_NEB_adapter.fa", "-t", "2"], "input": "mixed.fq"},
        {"name": "adapter_r1_only", "program": "clean_adapter", "args": ["-a", "illumina_NEB_adapter_R1.fa", "-b", "1", "-s", "20", "-r", "0"],
         "input": "mixed.fq.gz"},
        {"name": "adapter_norecords", "program": "clean_adapter", "args": ["-a", "illumina_NEB_adapter.fa"], "input": "norecords.fq"},
        {"name": "lowqual_default", "program": "clean_lowqual", "args": [], "input": "reads.fq"},
        {"name": "lowqual_e01", "program": "clean_lowqual", "args": ["-e", "0.01", "-r", "30", "-t", "2"], "input": "mixed.fq.gz"},
        {"name": "lowqual_mixed_plain", "program": "clean_lowqual", "args": ["-e", "0.05", "-r", "0"], "input": "mixed.fq"},
        {"name": "lowqual_phred64", "program": "clean_lowqual", "args": ["-q", "64"], "input": "phred64.fq"},
        {"name": "lowqual_norecords", "program": "clean_lowqual", "args": [], "input": "norecords.fq"},
    ]
    for case in cases:
        d = os.path.join(OUT, case["name"])
        os.makedirs(d)
        subprocess.run([os.path.join(ref, case["program"])] + case["args"] + [case["input"], os.path.join(case["name"], "out.gz"),
                                                                             os.path.join(case["name"], "out.stat")],
                       cwd=OUT, check=True, capture_output=True, timeout=600)
        want, got = CR.expected_outputs(OUT, case), CR.run_case(OUT, case)
        assert got["out"] == want["out"] and got["stat"] == want["stat"], "the restatement differs from the reference: " + case["name"]
        if case["program"] == "clean_adapter" and "norecords" not in case["name"] and "r1_only" not in case["name"]:
            missing = [c for c in CR.NEED_ADAPTER if c not in CR.adapter_coverage(OUT, case)]
            assert not missing, (case["name"], missing)
    json.dump(cases, open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    for prog in ("clean_adapter", "clean_lowqual"):
        r = subprocess.run([os.path.join(ref, prog)], capture_output=True, check=True)
        open(os.path.join(HERE, "clean_usage_%s.txt" % prog.split("_")[1]), "wb").write(r.stdout)
    sizes = {f: os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(OUT) for f in fs}
    print("wrote %d files, largest %d bytes" % (len(sizes), max(sizes.values())))


if __name__ == "__main__":
    main()
