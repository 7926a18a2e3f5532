"""Generate the link_scaffold golden vectors with the REAL reference program.  tests/golden/link_cases/ holds cases.json (per
case: options, output prefix, contig file or lengths file, library file, tie flag) and per case one archive <case>.zip (written
with fixed dates) with the inputs (contig FASTA or a names-and-lengths table, the .lib file, the 2ctg map files as gz written with
mtime=0) and expected/ with everything the reference wrote: its six output files under their own names and stderr.txt without
the `Run time:` lines.
link_usage.txt is the usage text.  The fixtures are data; this script needs the reference only when it is run:

    python tests/golden/make_link_golden.py /path/to/link_scaffold [/path/to/reference/test]

The program is the reference's link_scaffold built by its Makefile (link_scaffold/Makefile; it needs Boost), or the x86-64 binary
the reference ships as link_scaffold/link_scaffold.  With the reference's test directory as second argument the two E. coli runs
of test/03.build_scaffold are (re)made as well, and the program is asserted to reproduce the shipped results: all six files of
the insert-800 run, the four that depend on contig lengths only of the insert-400 run (its contig FASTA is not shipped; the
lengths are, and placeholder sequences of those lengths stand in).  Only the map files, the lengths and those four outputs are
stored for them.

Every synthetic case is asserted to show what it is meant to pin (see `expect` in scenario()), the untied cases to have no two
scaffolds and no two repeat nodes of one length, and tests/link_restatement.py to equal the program on every case."""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import link_restatement as LR  # noqa: E402

OUT = os.path.join(HERE, "link_cases")
WORK = tempfile.mkdtemp()        # the cases as directories, packed into OUT/<case>.zip


def pack(case):
    d = os.path.join(WORK, case["name"])
    with zipfile.ZipFile(os.path.join(OUT, case["name"] + ".zip"), "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for root, _, files in sorted(os.walk(d)):
            for f in sorted(files):
                info = zipfile.ZipInfo(os.path.relpath(os.path.join(root, f), d), date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                z.writestr(info, open(os.path.join(root, f), "rb").read())


def write_gz(path, data):
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:
        g.write(data)


class Scenario:
    """2ctg lines that make chosen links between oriented contigs, whatever -m and -i are"""

    def __init__(self, P, lens, rng):
        self.P, self.lens, self.rng, self.lines, self.n = P, lens, rng, [], 0

    def line(self, A, s1, e1, d1, B, s2, e2, d2):
        self.n += 1
        row = lambda tag, c, s, e, d: "read_%d/%d\t250\t1\t%d\tctg_%d\t%d\t%d\t%d\t%s\t%s%%" % (  # noqa: E731
            self.n, tag, max(1, abs(e - s) + 1), 2 * c + 1, self.lens[c], s, e, d, "100" if self.n % 3 else "98.7234")
        self.lines.append(row(1, A, s1, e1, d1) + "\t" + row(2, B, s2, e2, d2))

    def record(self, cls, A, B, gap):
        """one record of class cls, mate 1 on contig A and mate 2 on B, whose gap comes out as `gap` (link_func.cpp:262-313, :367-415)"""
        I, L = self.P.i, self.lens
        t1 = int(self.rng.integers(20, 60))
        t2 = I - gap - t1
        tail = lambda c, t: (L[c] - t, L[c] - t + 99)   # a term  len - start  # noqa: E731
        head = lambda t: (t - 99, t)                    # a term  end          # noqa: E731
        pe = self.P.m == 0
        if cls == ("FR" if pe else "RF"):
            a, b = tail(A, t1), head(t2)
        elif cls == ("RF" if pe else "FR"):
            a, b = head(t2), tail(B, t1)
        elif cls == ("FF" if pe else "RR"):
            a, b = tail(A, t1), tail(B, t2)
        else:
            a, b = head(t1), head(t2)
        self.line(A, a[0], a[1], cls[0], B, b[0], b[1], cls[1])

    def link(self, X, ox, Y, oy, gaps, alt=False):
        """records that add node X(ox) -> Y(oy), and with it rev(Y) -> rev(X); alt: the other class that gives + -> +"""
        pe = self.P.m == 0
        for g in gaps:
            if (ox, oy) == ("+", "+"):
                if alt:
                    self.record("RF" if pe else "FR", Y, X, g)
                else:
                    self.record("FR" if pe else "RF", X, Y, g)
            elif (ox, oy) == ("+", "-"):
                self.record("FF" if pe else "RR", X, Y, g)
            elif (ox, oy) == ("-", "+"):
                self.record("RR" if pe else "FF", X, Y, g)
            else:
                self.link(Y, "+", X, "+", [g], alt)


N_CONTIGS = 36


def make_contigs(rng, tie):
    lens = [int(x) for x in rng.choice(np.arange(400, 3000), N_CONTIGS, replace=False)]
    lens[12] = 60                                      # the middle contigs of the two interleave triples
    lens[28] = 75
    lens[33] = 1                                       # a contig of one base
    if tie:
        lens[31] = lens[30]                            # two one-contig scaffolds and two repeat nodes of one length
        lens[18] = lens[8]
    seqs = ["".join("ACGT"[v] for v in rng.integers(0, 4, n)) for n in lens]
    s = seqs[2]                                        # reversed in its scaffold: lower case, N / n, IUPAC and other letters
    seqs[2] = s[:10] + "acgtnNRYKMSWBDHVryU-*x" + s[32:100].lower() + s[100:]
    seqs[1] = seqs[1][:50] + "NNNNNnnnn" + seqs[1][59:]
    return lens, seqs


def fasta(lens, seqs):
    out = []
    for c, s in enumerate(seqs):
        out.append(">ctg_%d%s\n" % (2 * c + 1, "  length:%d\tmore" % lens[c] if c % 3 == 0 else ""))
        width = 70 if c % 4 == 1 else len(s)           # some sequences over several lines
        out += [s[p:p + width] + "\n" for p in range(0, len(s), width)]
    return "".join(out)


def scenario(P, lens, rng, big):
    S = Scenario(P, lens, rng)
    I = P.i
    # (a) a chain 0+ 1+ 2- 3+ through three classes: a negative sum with a non-exact average (-123 / 4 = -30, floor would be -31)
    #     and gaps <= 0 that are written as 1; contig 2 is written reverse-complemented
    S.link(0, "+", 1, "+", [25, 24, 27, 25, 26])
    S.link(1, "+", 2, "-", [-30, -31, -30, -32])
    S.link(2, "-", 3, "+", [0, 0, 1])
    # (b) + -> + through the other class
    S.link(4, "+", 5, "+", [10, 11, 13], alt=True)
    # (c) wrong directions: a letter that is neither F nor R, and two letters
    S.line(0, 100, 199, "N", 1, 1, 100, "R")
    S.line(0, 100, 199, "F", 1, 1, 100, "FR")
    S.line(0, 100, 199, "f", 1, 1, 100, "R")
    # (d) the gap filter's edges: -I/2 and I + 1 are dropped, -I/2 + 1 and I are kept (2 records: below the default -n)
    S.link(6, "+", 7, "+", [-(I // 2), -(I // 2) + 1, I, I + 1])
    # (e) a node with three links, first seen in the order 20, 10, 15, and one more of a single record (cleared by -n 3; the source
    #     then is a repeat node, so remove_links_from_deleted_nodes meets the cleared entry and counts it again)
    for t in (20, 10, 15, 10, 20, 15, 15, 20, 10):
        S.link(8, "+", t, "+", [40 + t])
    S.link(8, "+", 21, "+", [33])
    # (f) interleaving: start 11+ has the links middle 12+ (first) and end 13+; end 13- sees start first, then middle: the start
    #     takes the first branch (link_func.cpp:553-564), the end's reverse the second (:566-577)
    S.link(11, "+", 12, "+", [20, 21, 19])
    S.link(11, "+", 13, "+", [150, 151, 149])
    S.link(12, "+", 13, "+", [20, 20, 22])
    #     ... and the mirror image: start 27+ sees the end first (second branch), end 29- the middle first (first branch)
    S.link(28, "+", 29, "+", [20, 21, 19])
    S.link(27, "+", 29, "+", [150, 151, 149])
    S.link(27, "+", 28, "+", [20, 20, 22])
    # (g) a node with two incoming links
    S.link(16, "+", 18, "+", [5, 6, 7])
    S.link(17, "+", 18, "+", [50, 60, 70])
    # (i) a circle
    S.link(22, "+", 23, "+", [15, 15, 15])
    S.link(23, "+", 24, "-", [16, 15, 15])
    S.link(24, "-", 22, "+", [17, 15, 15])
    #     a chain that starts reversed and contains the contig of one base
    S.link(32, "-", 33, "-", [3, 4, 5])
    S.link(33, "-", 34, "+", [300, 310, 320])
    if big:
        # (l) a link stops counting at 1023 records: the sum covers the first 1023 in record order
        S.link(25, "+", 26, "+", [-50] * 1023 + [-150] * 77)
    return S.lines


CASES = [  # name, args, tie, big
    ("pe_default", [], False, True),
    ("mp_default", ["-m", "1", "-i", "500"], False, True),
    ("pe_n0", ["-n", "0"], False, False),
    ("pe_n1", ["-n", "1", "-m", "0"], False, False),
    ("pe_i401", ["-i", "401", "-n", "2"], False, False),
    ("mp_i301_n1", ["-m", "1", "-i", "301", "-n", "1"], False, False),
    ("pe_tie", ["-i", "400"], True, False),
]


def run_reference(prog, case, workdir, contig_file):
    P = LR.case_params(case)
    r = subprocess.run([prog] + case["args"] + ["-o", case["prefix"], contig_file, case["lib"]], cwd=workdir, capture_output=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for kind in LR.OUTPUTS:
        name = LR.output_name(case, P, kind)
        got[name] = open(os.path.join(workdir, name), "rb").read()
        os.remove(os.path.join(workdir, name))
    got["stderr.txt"] = LR.strip_run_time(r.stderr.decode("latin-1")).encode("latin-1")
    return got


def store_expected(case, got, keep=None):
    d = os.path.join(WORK, case["name"], "expected")
    os.makedirs(d, exist_ok=True)
    for name, data in got.items():
        if keep is None or any(name.endswith(k) for k in keep):
            open(os.path.join(d, name), "wb").write(data)


def check_restatement(case):
    pack(case)
    want = LR.expected_outputs(OUT, case)
    got, res = LR.run_case(OUT, case)
    assert sorted(got) == sorted(want), (case["name"], sorted(got), sorted(want))
    for f in want:
        if case.get("tie") and not f.endswith(("links.all", "links.uniq", "stderr.txt")):
            assert LR.split_records(got[f]) == LR.split_records(want[f]), (case["name"], f)
        else:
            assert got[f] == want[f], (case["name"], f)
    return res


def synthetic(prog):
    cases = []
    for n, (name, args, tie, big) in enumerate(CASES):
        rng = np.random.default_rng(100 + n)
        case = {"name": name, "args": args, "prefix": "res_" + name, "contigs": "contigs.fa", "lib": "pairs.lib", "tie": tie}
        P = LR.case_params(case)
        lens, seqs = make_contigs(rng, tie)
        lines = scenario(P, lens, rng, big)
        d = os.path.join(WORK, name)
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        open(os.path.join(d, "contigs.fa"), "w").write(fasta(lens, seqs))
        cut = len(lines) // 3
        header = "#read_id\tread_length\t...\n"
        write_gz(os.path.join(d, "part1.2ctg.gz"), (header + "\n".join(lines[:cut]) + "\n").encode())
        write_gz(os.path.join(d, "part2.2ctg.gz"), (header + "\n".join(lines[cut:]) + "\n").encode())
        open(os.path.join(d, "pairs.lib"), "w").write("# the map files of this library\n\npart1.2ctg.gz\tignored words\n#skipped.gz\n  part2.2ctg.gz\n")
        got = run_reference(prog, case, d, "contigs.fa")
        store_expected(case, got)
        res = check_restatement(case)
        c = res["counters"]
        # what the case is there to pin shows in the program's own output
        allf = got[LR.output_name(case, P, "scaffold.links.all")].decode()
        assert min(c["FR"], c["RF"], c["FF"], c["RR"]) > 0 and c["wrong"] == 3, c
        assert c["interleave"] == 4 and c["repeat"] >= 2, c
        assert (",4,-123,-30" in allf) == (P.n <= 4)
        rows = {int(l.split("\t")[0]): l.rstrip("\n").split("\t") for l in allf.splitlines()[1:]}
        assert [t.split(",")[0] for t in rows[17][3:7]][:3] == ["41", "21", "31"], rows[17]
        if P.n <= 2:
            assert rows[13][3].split(",")[1] == "2", rows[13]                       # the gap filter kept 2 of the 4 records
        if big:
            assert "53,1023,-51150,-50" in rows[51][3:], rows[51]
        if P.n == 3:
            assert c["lowfreq"] >= 2, c
        seq_fa = got[LR.output_name(case, P, "scaffold.seq.fa")].decode("latin-1")
        assert LR.reverse_complement(seqs[2]) in seq_fa and "N" + LR.reverse_complement(seqs[2]) + "N" in seq_fa   # gaps <= 0 as 1
        pos = got[LR.output_name(case, P, "scaffold.pos.tab")].decode()
        assert "\tctg_45\t" in pos and "\tctg_49\t" in pos                            # the circle is read out once
        lengths = [sum(int(lens[cc]) if cc is not None else b for cc, b in items) for items in res["layout"]]
        rep = [t.split("\t")[4] for t in got[LR.output_name(case, P, "scaffold_repeat.pos.tab")].decode().splitlines() if t[:1] == "\t"]
        assert (len(set(lengths)) < len(lengths) and len(set(rep)) < len(rep)) == tie, (name, "ties")
        if not tie:
            assert len(set(lengths)) == len(lengths) and len(set(rep)) == len(rep), (name, "ties")
        cases.append(case)
        print(name, c)
    return cases


def ecoli(prog, ref_test):
    base = os.path.join(ref_test, "03.build_scaffold")
    runs = [
        ("ecoli_insert400", "400", "scaffold_with_insert400", os.path.join(ref_test, "02.build_contig", "Ecoli_corrected_reads.contig.seq.fa.len"),
         "Ecoli_corrected_reads.contig", None, dict(effective=6479, interleave=37, repeat=78, scaffolds=131)),
        ("ecoli_insert800", "800", "scaffold_with_insert800",
         os.path.join(base, "scaffold_with_insert400", "Ecoli_corrected_reads.contig.insert400.scaffold.seq.fa.len"),
         "Ecoli_corrected_reads.contig.insert400.scaffold",
         os.path.join(base, "scaffold_with_insert400", "Ecoli_corrected_reads.contig.insert400.scaffold.seq.fa"),
         dict(effective=769, interleave=0, repeat=8, scaffolds=90)),
    ]
    keep = ("links.all", "links.uniq", "scaffold.pos.tab", "scaffold_repeat.pos.tab", "stderr.txt")
    cases = []
    for name, insert, sub, len_file, prefix, real_fasta, counts in runs:
        case = {"name": name, "args": ["-i", insert], "prefix": prefix, "lengths": "contigs.len", "lib": "pairs.lib", "tie": False}
        P = LR.case_params(case)
        d = os.path.join(WORK, name)
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        shutil.copy(len_file, os.path.join(d, "contigs.len"))
        os.chmod(os.path.join(d, "contigs.len"), 0o644)
        maps = [f for f in os.listdir(os.path.join(base, sub, "maping_results")) if f.endswith(".2ctg.gz")]
        assert len(maps) == 1
        write_gz(os.path.join(d, "pairs.2ctg.gz"), gzip.open(os.path.join(base, sub, "maping_results", maps[0])).read())
        open(os.path.join(d, "pairs.lib"), "w").write("pairs.2ctg.gz\n")
        names, lens = zip(*[(t.split()[0], int(t.split()[1])) for t in open(len_file) if t.strip()])
        with tempfile.TemporaryDirectory() as tmp:
            for f in ("pairs.2ctg.gz", "pairs.lib"):
                shutil.copy(os.path.join(d, f), tmp)
            with open(os.path.join(tmp, "placeholder.fa"), "w") as f:
                for nm, n in zip(names, lens):
                    f.write(">%s\n%s\n" % (nm, "A" * n))
            got = run_reference(prog, case, tmp, "placeholder.fa")
            shipped = os.path.join(base, sub)
            for kind in LR.OUTPUTS:
                fn = LR.output_name(case, P, kind)
                if fn.endswith(keep):
                    assert got[fn] == open(os.path.join(shipped, fn), "rb").read(), (name, fn)
            if real_fasta:                                                          # all six with the real sequences
                shutil.copy(real_fasta, os.path.join(tmp, "real.fa"))
                full = run_reference(prog, case, tmp, "real.fa")
                for kind in LR.OUTPUTS:
                    fn = LR.output_name(case, P, kind)
                    assert full[fn] == open(os.path.join(shipped, fn), "rb").read(), (name, fn)
        store_expected(case, got, keep)
        res = check_restatement(case)
        c = res["counters"]
        assert (c["FR"] + c["RF"] + c["FF"] + c["RR"], c["interleave"], c["repeat"], c["scaffolds"]) == \
            (counts["effective"], counts["interleave"], counts["repeat"], counts["scaffolds"]), c
        case["counters"] = c
        cases.append(case)
        print(name, c)
    return cases


def main():
    prog = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    usage = subprocess.run([prog, "-h"], capture_output=True).stdout
    assert usage == subprocess.run([prog], capture_output=True).stdout and usage
    open(os.path.join(HERE, "link_usage.txt"), "wb").write(usage)
    cases = synthetic(prog)
    path = os.path.join(OUT, "cases.json")
    if len(sys.argv) > 2:
        cases += ecoli(prog, os.path.abspath(sys.argv[2]))
    elif os.path.exists(path):
        cases += [c for c in json.load(open(path)) if "lengths" in c]
    open(path, "w").write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    shutil.rmtree(WORK)


if __name__ == "__main__":
    main()
