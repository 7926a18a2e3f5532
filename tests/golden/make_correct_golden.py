"""Generate the correct_error_reads golden vectors with the REAL reference program.  Each case directory
tests/golden/correct_<table>/ holds one 1-bit k-mer table (table.cz + table.cz.len, the format kmerfreq -b 1
writes), the read files, cases.json (per case: the reads file, its format and the options) and, per case, the
reference's <case>.correct.fa.gz (recompressed without a time stamp) and its <case>.correct.stat; correct_usage.txt is
its usage text.  The fixtures are data; this script needs the reference only when it is run.

The binary is built from the files of the reference Makefile's rule (correct_error/Makefile:9-10), with the
main file at -O0: at -O3 the 1-bit loader, which falls off the end of non-void functions, crashes on start-up.

    g++ -O0 -c main_parallel_senior.cpp -o main.o
    g++ -O3 -o correct_error_reads seqKmer.cpp main.o correct.cpp gzstream.cpp -lz -lpthread

    python tests/golden/make_correct_golden.py /path/to/correct_error_reads
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import oracle_py as orc  # noqa: E402

BLOCK_BYTES = 1 << 20  # 8 Mi k-mers per compressed block (SrcBlockSize / 8)


def rc_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def kmer_val(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def genome_table(genome, reads, k, cutoff):
    """raw 1-bit file content: bit of canonical v set when v occurs more than cutoff times in reads (ACGT only)"""
    counts = {}
    for r in reads:
        u = r.upper()
        for i in range(len(u) - k + 1):
            w = u[i:i + k]
            if any(ch not in "ACGT" for ch in w):
                continue
            v = min(kmer_val(w), kmer_val(rc_str(w)))
            counts[v] = counts.get(v, 0) + 1
    bits = np.zeros(max(4 ** k // 8, 1), dtype=np.uint8)
    for v, n in counts.items():
        if n > cutoff:
            bits[v >> 3] |= 0x80 >> (v & 7)
    return bits


def mutate(rng, s, err, n_rate=0.0, lower_rate=0.0):
    out = list(s)
    for i in range(len(out)):
        u = rng.random()
        if u < err:
            out[i] = "ACGT"[("ACGT".index(out[i]) + 1 + rng.integers(3)) % 4]
        elif u < err + n_rate:
            out[i] = "N"
        elif u < err + n_rate + lower_rate:
            out[i] = out[i].lower()
    return "".join(out)


def sample(rng, genome, n, lengths, err, n_rate=0.002, lower_rate=0.002):
    reads = []
    for i in range(n):
        L = int(lengths[i % len(lengths)])
        p = int(rng.integers(0, len(genome) - L))
        s = genome[p:p + L]
        if rng.random() < 0.5:
            s = rc_str(s)
        reads.append(mutate(rng, s, err, n_rate, lower_rate))
    return reads


def write_bytes(path, data, gz):
    """gzip without a time stamp, so that a rerun writes the same bytes"""
    with open(path, "wb") as f:
        if gz:
            with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
                z.write(data)
        else:
            f.write(data)


def write_fq(path, reads, gz=False):
    write_bytes(path, "".join("@r%d/1\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)).encode(), gz)


def write_fa(path, reads, gz=False):
    write_bytes(path, "".join(">r%d desc\n%s\n" % (i, s) for i, s in enumerate(reads)).encode(), gz)


def special_reads(rng, genome, k):
    """lengths 0, < k, = k, k + 1, 150, 250 and > 1000; lower case; N runs"""
    g = genome
    return ["", g[:k - 3], g[100:100 + k], g[200:200 + k + 1], mutate(rng, g[300:1500], 0.01),
            g[2000:2150].lower(), mutate(rng, g[3000:3150], 0.02).lower(), g[4000:4060] + "NNNN" + g[4064:4150],
            g[5000:5150], "N" * 150, mutate(rng, g[6000:6250], 0.01), g[7000:7075] + "nn" + g[7077:7150]]


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    # k = 13: default options pin the "-m / -x are 17 whatever -k" rule
    g13 = "".join(rng.choice(list("ACGT"), size=20000))
    base = sample(rng, g13, 1200, [150, 150, 100, 250], 0.01)
    table13 = genome_table(g13, base, 13, 1)
    sp = special_reads(rng, g13, 13)
    out.append(("k13", 13, table13, [
        ("default", "reads.fq.gz", 1, [], base[:400] + sp, "fq.gz"),
        ("c0", "reads.fq.gz", 1, ["-c", "0"], None, None),
        ("c3_m20_x5_r50", "reads.fq.gz", 1, ["-c", "3", "-m", "20", "-x", "5", "-r", "50"], None, None),
        ("fasta_m9_r0", "small.fa.gz", 2, ["-m", "9", "-r", "0"], base[400:450] + sp, "fa.gz"),
    ]))
    # even k: palindromic k-mers go through the mirror rule
    g12 = "".join(rng.choice(list("ACGT"), size=12000))
    g12 = g12[:5000] + "ACGTACGTACGTACGTACGT" + rc_str(g12[5000:5100]) + g12[5100:]
    r12 = sample(rng, g12, 500, [150, 100], 0.01)
    out.append(("k12", 12, genome_table(g12, r12, 12, 1), [("default", "reads.fq.gz", 1, ["-m", "12", "-x", "12"], r12[:250], "fq.gz")]))
    # a dense table (the genome's k-mers plus 90 % of all bits): wide trees; a small -n hits the node limit
    g9 = "".join(rng.choice(list("ACGT"), size=4000))
    r9 = sample(rng, g9, 150, [100, 150], 0.03)
    bits9 = genome_table(g9, r9, 9, 0) | np.packbits((rng.random(4 ** 9) < 0.9).astype(np.uint8))
    out.append(("k9_dense", 9, bits9, [
        ("n4000", "reads.fq.gz", 1, ["-m", "9", "-x", "9", "-r", "40", "-n", "4000"], r9, "fq.gz"),
        ("n60_c3", "reads.fq.gz", 1, ["-m", "12", "-c", "3", "-n", "60"], None, None),
    ]))
    return out


def main():
    exe = os.path.abspath(sys.argv[1])
    usage = subprocess.run([exe], capture_output=True, timeout=60).stdout   # the usage text (no arguments)
    open(os.path.join(HERE, "correct_usage.txt"), "wb").write(usage)
    for tname, k, raw, clist in cases():
        d = os.path.join(HERE, "correct_" + tname)
        os.makedirs(d, exist_ok=True)
        orc.kfreq_write_cz(os.path.join(d, "table.cz"), raw.tobytes(), BLOCK_BYTES)
        meta = []
        for cname, rfile, fmt, opts, reads, kind in clist:
            if reads is not None:
                w = write_fq if kind.startswith("fq") else write_fa
                w(os.path.join(d, rfile), reads, gz=kind.endswith(".gz"))
            args = ["-k", str(k), "-t", "4", "-f", str(fmt)] + opts
            with tempfile.TemporaryDirectory() as tmp:
                shutil.copy(os.path.join(d, rfile), os.path.join(tmp, rfile))
                with open(os.path.join(tmp, "reads.lib"), "w") as f:
                    f.write(" %s \n" % os.path.join(tmp, rfile))
                r = subprocess.run([exe] + args + [os.path.join(d, "table.cz"), os.path.join(tmp, "reads.lib")],
                                   capture_output=True, text=True, check=True, timeout=600)
                fa = gzip.open(os.path.join(tmp, rfile + ".correct.fa.gz"), "rb").read()
                stat = open(os.path.join(tmp, rfile + ".correct.stat")).read()
            write_bytes(os.path.join(d, cname + ".correct.fa.gz"), fa, True)
            open(os.path.join(d, cname + ".correct.stat"), "w").write(stat)
            hits = r.stderr.count("node_vec_pos exceed Max_node_in_BB_tree")
            hif = int(r.stderr.split("Kmer_hifreq_num")[1].split()[0])
            meta.append({"name": cname, "reads": rfile, "format": fmt, "args": args, "k": k,
                         "node_limit_hits": hits, "hifreq": hif})
            print(tname, cname, "hits", hits, "hifreq", hif, stat.split("\n")[8:10])
        with open(os.path.join(d, "cases.json"), "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(m) for m in meta) + "\n]\n")


if __name__ == "__main__":
    main()
