"""Generate the map_reads / map_pair golden vectors with the REAL reference programs.  tests/golden/map_cases/ holds one contig
file, the read files (gz ones written with mtime=0), the library files, cases.json (per case: program, options, contig file,
library file) and per case a directory <case>/ with everything the reference wrote: the gz outputs recompressed with mtime=0,
the .stat files and the .2ctg.lib file (its -o prefix replaced by OUT).  map_usage_reads.txt and map_usage_pair.txt are the two
usage texts.  The fixtures are data; this script needs the reference only when it is run.

The binaries are built with the reference Makefile's rule (link_scaffold/Makefile:3-8), kmerSet.cpp at -O0 (functions there
fall off the end of non-void functions, as in oracle/Makefile):

    g++ -O0 -w -c kmerSet.cpp -o kmerSet.o
    g++ -O2 -w -o map_reads kmerSet.o map_func.cpp seqKmer.cpp gzstream.cpp map_reads.cpp -lz -lpthread
    g++ -O2 -w -o map_pair  kmerSet.o map_func.cpp seqKmer.cpp gzstream.cpp map_pair.cpp  -lz -lpthread

    python tests/golden/make_map_golden.py /path/to/map_reads /path/to/map_pair [cases | edges]

Every category the tests rely on is asserted here to be present in the reference's output (map_restatement.coverage).

tests/golden/map_edge_cases/ is a second set (written with `edges`, or with both when no third argument is given): the crafted
scenarios of tests/map_edge_cases.py at (k, s) = (31, 5), (21, 5), (15, 40) and (31, 1), without bytes from 128 on.  Per (k, s)
one contig file; per scenario the reads as gzipped FASTA and two library files (the one of map_pair names the reads file twice:
every read is its own mate), and two cases, <scenario>__reads and <scenario>__pair.  What the reference wrote for a case is
kept as one file, <case>.out.json.gz: {output file name: text}, in the form map_restatement.expected_outputs gives."""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import map_restatement as MR  # noqa: E402

K, S = 31, 5
RC = str.maketrans("ACGTacgt", "TGCAtgca")


def rand_seq(rng, n):
    return "".join("ACGT"[v] for v in rng.integers(0, 4, n))


def mutate(rng, s, rate):
    return "".join("ACGT"[("ACGT".index(c) + int(rng.integers(1, 4))) % 4] if c in "ACGT" and rng.random() < rate else c for c in s)


def write_gz(path, data):
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:
        g.write(data)


def write_reads(path, reads, fmt):
    text = "".join(("@%s\n%s\n+\n%s\n" % (h, s, "I" * len(s))) if fmt == 1 else (">%s\n%s\n" % (h, s)) for h, s in reads)
    if path.endswith(".gz"):
        write_gz(path, text.encode())
    else:
        open(path, "w").write(text)


def make_contigs(rng):
    g = rand_seq(rng, 6400)     # pieces of one genome: reads over a cut between adjacent pieces map to two contigs
    rep = rand_seq(rng, 220)    # the same piece in two contigs: its k-mers have freq == 0
    return g, {"ctgA": g[0:900] + rep + g[900:1800], "ctgB": g[1800:3400], "ctgC_lower": g[3400:4400].lower(),
               "scaf": g[4400:5000] + "N" * 60 + g[5060:5600],   # a scaffold: windows of the index never span the gap
               "tiny": g[5600:5680],                              # shorter than -l: keeps its index, becomes empty
               "ctgD": g[5680:5900] + rep + g[5900:6400],
               "circ": rand_seq(rng, 900),                        # read out as a circle: reads cross its junction
               "polyA": rand_seq(rng, 150) + "C" + "A" * K + "G" + rand_seq(rng, 250)}  # its only all-A window is unique (key 0)


def sample_reads(rng, g, ctg, n, lo, hi, sub, tag):
    """single reads of every kind -> [(header, sequence)]"""
    out = []
    for i in range(n):
        L, kind = int(rng.integers(lo, hi + 1)), i % 12
        cut_len = lambda: int(rng.integers(L // 4, 3 * L // 4))  # noqa: E731
        if kind < 4:                                # inside one contig (or all of it)
            s = ctg[["ctgA", "ctgB", "ctgC_lower", "scaf", "ctgD", "polyA"][int(rng.integers(0, 6))]]
            p = int(rng.integers(0, max(1, len(s) - L)))
            r = s[p:p + L]
        elif kind in (4, 5):                        # over the cut between ctgA's and ctgB's genome pieces, and B | C
            p = (1800 if kind == 4 else 3400) - cut_len()
            r = g[p:p + L]
        elif kind == 6:                             # over the junction of the circle: both parts on one contig
            a = min(cut_len(), 600)
            r = ctg["circ"][len(ctg["circ"]) - a:] + ctg["circ"][:min(L - a, 600)]
        elif kind == 7:                             # nothing to map
            r = rand_seq(rng, L)
        elif kind == 8:                             # over a cut, the second part too divergent for -i
            a = int(rng.integers(L // 3, L // 2))
            tail = g[1800:1800 + L - a]
            r = g[1800 - a:1800] + tail[:45] + mutate(rng, tail[45:], 0.2)
        elif kind == 9:                             # starts in the repeat
            r = ctg["ctgD"][225 + int(rng.integers(0, 100)):][:L]
        elif kind == 10:                            # starts at the unique all-A window
            r = ctg["polyA"][151:151 + L]
        else:                                       # scaffold, across the N gap
            p = 600 - cut_len()
            r = ctg["scaf"][max(p, 0):p + L]
        if kind != 8:
            r = mutate(rng, r, sub)
        if i % 7 == 3:                              # N, lower case and letters outside the alphabet
            r = list(r)
            for _ in range(3):
                r[int(rng.integers(0, len(r)))] = "NnRYK-."[int(rng.integers(0, 7))]
            q = int(rng.integers(0, len(r) - 20))
            r[q:q + 20] = "".join(r[q:q + 20]).lower()
            r = "".join(r)
        out.append(("%s_%d%s" % (tag, i, " desc/1" if i % 5 == 0 else ""), r[::-1].translate(RC) if i % 2 else r))
    return out


def sample_pairs(rng, g, ctg, n, L, sub, tag):
    a, b = [], []
    for i in range(n):
        kind = i % 5
        if kind < 2:                                # both mates on one contig
            s = ctg[["ctgB", "ctgC_lower", "ctgA"][i % 3]]
            p = int(rng.integers(0, len(s) - 3 * L))
            r1, r2 = s[p:p + L], s[p + 2 * L:p + 3 * L][::-1].translate(RC)
        elif kind == 2:                             # on two contigs
            p = 1800 - int(rng.integers(L + 50, 2 * L))
            r1, r2 = g[p:p + L], g[1900:1900 + L][::-1].translate(RC)
        elif kind == 3:                             # one mate maps
            p = int(rng.integers(0, len(ctg["ctgB"]) - L))
            r1, r2 = ctg["ctgB"][p:p + L], rand_seq(rng, L)
            r1, r2 = (r1, r2) if i % 2 else (r2, r1)
        else:
            r1, r2 = rand_seq(rng, L), rand_seq(rng, L)
        a.append(("%s_%d/1" % (tag, i), mutate(rng, r1, sub)))
        b.append(("%s_%d/2 second" % (tag, i), mutate(rng, r2, sub)))
    return a, b


def run_reference(exe, D, case):
    tmp = tempfile.mkdtemp(prefix="mapgold_")
    o = os.path.join(tmp, "o")
    subprocess.run([exe] + case["args"] + ["-o", o, case["contigs"], case["lib"]], cwd=D, check=True, timeout=1800,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    C = os.path.join(D, case["name"])
    os.makedirs(C)
    for f in sorted(os.listdir(o)):
        data = open(os.path.join(o, f), "rb").read()
        if f.endswith(".gz"):
            write_gz(os.path.join(C, f), gzip.decompress(data))
        else:
            open(os.path.join(C, f), "wb").write(data)
    lib_out = "%s.%s.2ctg.lib" % (case["lib"], case["program"])
    open(os.path.join(C, lib_out), "w").write(open(os.path.join(D, lib_out)).read().replace(o + "/", "OUT/"))
    os.remove(os.path.join(D, lib_out))
    shutil.rmtree(tmp)


def main_edges(exe):
    import map_edge_cases as E
    D = os.path.join(HERE, "map_edge_cases")
    shutil.rmtree(D, ignore_errors=True)
    os.makedirs(D)
    cases = []
    for scn in E.golden_scenarios():
        ctg = "contigs_k%ds%d.fa" % (scn.k, scn.s)
        text = "".join(">c%d\n%s\n" % (n, q.decode()) for n, q in enumerate(scn.contigs))
        assert not os.path.exists(os.path.join(D, ctg)) or open(os.path.join(D, ctg)).read() == text
        open(os.path.join(D, ctg), "w").write(text)
        write_reads(os.path.join(D, scn.name + ".fa.gz"), [("r%d" % n, q.decode()) for n, q in enumerate(scn.reads)], 2)
        open(os.path.join(D, scn.name + ".lib"), "w").write(scn.name + ".fa.gz\n")
        open(os.path.join(D, scn.name + ".pe.lib"), "w").write("%s.fa.gz\n%s.fa.gz\n" % (scn.name, scn.name))
        args = ["-k", str(scn.k), "-s", str(scn.s), "-r", str(scn.r), "-i", repr(scn.identity), "-f", "2", "-l", "100"]
        cases.append(dict(name=scn.name + "__reads", scenario=scn.name, program="map_reads", args=args, contigs=ctg, lib=scn.name + ".lib"))
        cases.append(dict(name=scn.name + "__pair", scenario=scn.name, program="map_pair", args=args, contigs=ctg, lib=scn.name + ".pe.lib"))
    open(os.path.join(D, "cases.json"), "w").write("[\n" + ",\n".join(" " + json.dumps(c) for c in cases) + "\n]\n")
    for case in cases:
        run_reference(exe[case["program"]], D, case)
        write_gz(os.path.join(D, case["name"] + ".out.json.gz"), json.dumps(MR.expected_outputs(D, case), sort_keys=True).encode())
        shutil.rmtree(os.path.join(D, case["name"]))


def main():
    exe = {"map_reads": os.path.abspath(sys.argv[1]), "map_pair": os.path.abspath(sys.argv[2])}
    which = sys.argv[3] if len(sys.argv) > 3 else "both"
    if which in ("edges", "both"):
        main_edges(exe)
    if which == "edges":
        return
    for prog, name in (("map_reads", "map_usage_reads.txt"), ("map_pair", "map_usage_pair.txt")):
        open(os.path.join(HERE, name), "wb").write(subprocess.run([exe[prog]], capture_output=True, timeout=60).stdout)
    rng = np.random.default_rng(11)
    D = os.path.join(HERE, "map_cases")
    shutil.rmtree(D, ignore_errors=True)
    os.makedirs(D)
    g, ctg = make_contigs(rng)
    with open(os.path.join(D, "contigs.fa"), "w") as f:
        for name, q in ctg.items():
            width = 100 if name in ("ctgA", "polyA") else len(q)   # two records span several lines
            f.write(">%s%s\n" % (name, " extra words" if name == "ctgA" else "\twith_gap" if name == "scaf" else ""))
            f.write("".join(q[j:j + width] + "\n" for j in range(0, len(q), width)))

    def lib(name, text):
        open(os.path.join(D, name), "w").write(text)

    se = sample_reads(rng, g, ctg, 240, 250, 320, 0.015, "se") + sample_reads(rng, g, ctg, 24, 1100, 1500, 0.01, "lng")
    write_reads(os.path.join(D, "se.fq.gz"), se + [("below_r", g[100:300])], 1)
    write_reads(os.path.join(D, "se2.fq"), sample_reads(rng, g, ctg, 12, 250, 300, 0.02, "pl"), 1)
    lib("se.lib", "# single reads\nse.fq.gz  insert=0 trailing tokens\n\n\tse2.fq\n")
    short = sample_reads(rng, g, ctg, 24, K + S - 1, K + S + 60, 0.01, "sh")
    for d in (-1, 0, 1):                              # k + s - 1, k + s and k + s + 1 bases
        short += [("polyA_edge%d" % d, ctg["polyA"][151:151 + K + S + d]), ("edge%d" % d, g[2000:2000 + K + S + d]),
                  ("edge_rc%d" % d, g[3000:3000 + K + S + d][::-1].translate(RC))]
    write_reads(os.path.join(D, "short.fa"), short, 2)
    lib("short.lib", "short.fa\n")
    for name, n, L, fmt in (("pe_%d.fq.gz", 150, 250, 1), ("pf_%d.fa", 10, 260, 2)):
        a, b = sample_pairs(rng, g, ctg, n, L, 0.015, name[:2])
        write_reads(os.path.join(D, name % 1), a, fmt)
        write_reads(os.path.join(D, name % 2), b, fmt)
    lib("pe.lib", "#pairs\npe_1.fq.gz 400\npe_2.fq.gz 400\n")
    lib("pf.lib", "pf_1.fa\npf_2.fa\n")
    k21 = ["-k", "21", "-s", "3", "-i", "0.9", "-l", "100"]
    cases = [dict(name=n, program=p, args=a, contigs="contigs.fa", lib=l) for n, p, a, l in (
        ("reads_default", "map_reads", ["-t", "3"], "se.lib"), ("reads_short", "map_reads", ["-f", "2", "-r", "30", "-t", "2"], "short.lib"),
        ("reads_k21", "map_reads", k21 + ["-r", "100"], "se.lib"), ("pair_default", "map_pair", [], "pe.lib"),
        ("pair_fasta", "map_pair", ["-f", "2"], "pf.lib"), ("pair_k21", "map_pair", k21 + ["-r", "120"], "pe.lib"))]
    open(os.path.join(D, "cases.json"), "w").write("[\n" + ",\n".join(" " + json.dumps(c) for c in cases) + "\n]\n")
    for case in cases:
        run_reference(exe[case["program"]], D, case)
    missing = [n for n in MR.NEED if n not in MR.coverage(D, cases)]
    assert not missing, missing


if __name__ == "__main__":
    main()
