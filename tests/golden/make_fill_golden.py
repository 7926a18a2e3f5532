"""Generate the link_contig golden vectors with the REAL reference program.  tests/golden/fill_cases/ holds cases.json (per case:
options, output prefix, contig file, library file) and per case one archive <case>.zip (written with fixed dates) with the inputs
(contig FASTA, the .lib file, the 2ctg map files and their .reads.fa.gz as gz written with mtime=0) and expected/ with everything
the reference wrote: its six output files under their own names and stderr.txt without the `Run time:` lines.  fill_usage.txt is
the usage text.  The fixtures are data; this script needs the reference only when it is run:

    python tests/golden/make_fill_golden.py /path/to/link_contig

The program is the reference's link_contig built by its Makefile (link_scaffold/Makefile; it needs Boost), or the x86-64 binary the
reference ships as link_scaffold/link_contig.  The fixtures here were written by the shipped binary; no difference between it and
the source (link_contig.cpp, link_func.cpp) showed in any case.

The inputs are what map_reads writes for reads laid over the junctions of oriented contigs: every spanning read is present and
long enough, so the reference stays inside defined behaviour.  Every case is asserted to show what it is meant to pin (see
checks()), and tests/fill_restatement.py to equal the program on every case."""
import gzip
import json
import re
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import fill_restatement as FR  # noqa: E402
import link_restatement as LR  # noqa: E402

OUT = os.path.join(HERE, "fill_cases")
WORK = tempfile.mkdtemp()
N_CONTIGS = 30
SHORT = 14                                             # a contig shorter than the overlap at its 3' end


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


def rand_seq(rng, n):
    return "".join("ACGT"[v] for v in rng.integers(0, 4, n))


class Scenario:
    """reads laid over the junction of two oriented contigs, and the 2ctg line map_reads writes for each"""

    def __init__(self, seqs, rng):
        self.seqs, self.rng, self.lines, self.reads, self.n = seqs, rng, [], [], 0

    def oriented(self, c, o):
        return self.seqs[c] if o == "+" else LR.reverse_complement(self.seqs[c])

    def read(self, X, ox, Y, oy, gap, filler="", reverse=False, d1=None, d2=None, name=None, arm=40):
        """one read: the last bases of X(ox), `filler` (gap > 0: gap bytes), the first bases of Y(oy); reverse: the read is the
        other strand, so its first alignment lies on Y.  d1 / d2 override the direction fields."""
        self.n += 1
        name = name or "read_%d" % self.n
        left, right = self.oriented(X, ox), self.oriented(Y, oy)
        la, lb = min(arm, len(left)), min(arm, len(right))
        assert len(filler) == max(gap, 0)
        if gap >= 0:
            seq = left[len(left) - la:] + filler + right[:lb]
        else:                                          # the alignments overlap on the read by -gap bases
            seq = left[len(left) - la:] + right[:lb] + rand_seq(self.rng, -gap)
        n = len(seq)
        e1, s2 = la, la + gap + 1                      # 1-based: alignment 1 is [1, e1], alignment 2 begins at s2
        flip = {"+": "-", "-": "+"}
        if reverse:
            seq = LR.reverse_complement(seq)
            e1, s2 = n - (la + max(gap, 0) + lb) + lb, 0
            # the read now begins with what follows Y's part: alignment 1 is Y's, it ends at e1; alignment 2 (X's) begins gap + 1 behind
            lead = n - (la + max(gap, 0) + lb)
            e1 = lead + lb
            s2 = e1 + gap + 1
            X, ox, Y, oy, la, lb = Y, flip[oy], X, flip[ox], lb, la
        D = {"+": "F", "-": "R"}
        d1, d2 = d1 or D[ox], d2 or D[oy]
        row = lambda rs, re, c, d: "%s\t%d\t%d\t%d\tctg_%d\t%d\t%d\t%d\t%s\t%s%%" % (  # noqa: E731
            name, n, rs, re, 2 * c + 1, len(self.seqs[c]), 1, max(re - rs + 1, 1), d, "100" if self.n % 3 else "98.5")
        self.lines.append(row(max(e1 - la + 1, 1), e1, X, d1) + "\t" + row(s2, min(s2 + lb - 1, n), Y, d2))
        self.reads.append((name, seq))
        return name

    def junction(self, X, ox, Y, oy, gaps, truth=None, **kw):
        """reads over X(ox) -> Y(oy) with the given gaps, alternately of either strand; those of one gap size share a filler"""
        fill = {}
        for k, g in enumerate(gaps):
            if g > 0 and g not in fill:
                fill[g] = truth if truth is not None and len(truth) == g else rand_seq(self.rng, g)
            self.read(X, ox, Y, oy, g, fill.get(g, ""), reverse=k % 2 == 1, **kw)
        return fill


def make_contigs(rng, tie):
    lens = [int(x) for x in rng.choice(np.arange(150, 700), N_CONTIGS, replace=False)]
    lens[9] = SHORT
    if tie:
        lens[27] = lens[26]                            # two one-contig scafftigs of one length
    seqs = [rand_seq(rng, n) for n in lens]
    seqs[2] = seqs[2][:60] + "acgtnNRYx" + seqs[2][69:]
    return seqs


def fasta(seqs):
    out = []
    for c, s in enumerate(seqs):
        out.append(">ctg_%d%s\n" % (2 * c + 1, "  length:%d" % len(s) if c % 3 == 0 else ""))
        width = 60 if c % 4 == 1 else len(s)
        out += [s[p:p + width] + "\n" for p in range(0, len(s), width)]
    return "".join(out)


def scenario(seqs, rng, big):
    S = Scenario(seqs, rng)
    # (a) a chain 0+ 1+ 2- 3+ 4+: positive gaps with one deviant read each, a zero gap, a negative gap
    S.junction(0, "+", 1, "+", [12, 12, 12, 12, 12, 14])
    S.junction(1, "+", 2, "-", [25, 25, 25, 25, 24])
    S.junction(2, "-", 3, "+", [0, 0, 0, 1])
    S.junction(3, "+", 4, "+", [-8, -8, -8, -7, -8])
    # (b) a mode tie: three reads of gap 10, three of gap 13: the smaller gap is the mode
    S.junction(5, "+", 6, "+", [13, 10, 13, 10, 13, 10])
    # (c) a column tie (two A, two C in column 2: A wins) and a minority base (column 5): identity below 1
    t = "GGTTGAC"
    for k, f in enumerate(("GGATGAC", "GGCTGAC", "GGATGTC", "GGCTGAC")):
        S.read(6, "+", 7, "+", 7, f, reverse=k % 2 == 1)
    for f in (t, t, t, t, "GGTTGAA", t):
        S.read(7, "+", 8, "-", 7, f, reverse=f != t)
    # (d) an overlap longer than the left contig: substr(0, negative) keeps all of contig 9
    S.junction(8, "-", 9, "+", [3, 3, 3])
    S.junction(9, "+", 10, "+", [-(SHORT + 6)] * 3, arm=SHORT)
    # (e) lower case, n and other bytes in the slices of a gap, forward and reversed reads among them
    for k, f in enumerate(("ACgTN", "ACgTN", "ACGTN", "acgtn", "ACRTN", "ACgTN")):
        S.read(11, "+", 12, "+", 5, f, reverse=k in (2, 4))
    #     ... and a gap whose consensus is N
    for f in ("ANNA", "ANCA", "ANNA"):
        S.read(12, "+", 13, "-", 4, f)
    # (f) records of conflicting orientations on one pair, pooled into one gap: 14+ -> 15+ four times, 14+ -> 15- once (below -n 3)
    fill = S.junction(14, "+", 15, "+", [9, 9, 9, 9])
    S.read(14, "+", 15, "-", 9, rand_seq(rng, 9))
    # (g) wrong directions: in the statistics and in the consensus, not in the links
    S.read(14, "+", 15, "+", 9, fill[9], d1="N")
    S.read(14, "+", 15, "+", 11, rand_seq(rng, 11), d2="FR")
    # (h) a node with two incoming links and one with two outgoing: repeat nodes
    S.junction(16, "+", 18, "+", [5, 5, 6, 5, 5])
    S.junction(17, "+", 18, "+", [8] * 5)
    S.junction(19, "+", 20, "+", [4] * 5)
    S.junction(19, "+", 21, "-", [6] * 5)
    # (i) links of 1, 2, 4 records: cut by -n 3 / -n 5
    S.junction(23, "+", 24, "+", [6, 6])
    S.junction(24, "+", 25, "-", [2, 2, 2, 2])
    if big:
        # (k) a link of more than 1023 records: the link stops counting, the statistics do not
        S.junction(28, "+", 29, "+", [3] * 1040 + [4] * 30, arm=25)
    # (j) a read id that occurs in both reads files: the later entry is the one used (the earlier has other bytes in the gap)
    S.read(22, "+", 23, "+", 7, "TTTTTTT", name="read_twice")
    return S


CASES = [  # name, args, tie, big
    ("n_default", [], False, True),
    ("n1", ["-n", "1"], False, False),
    ("n5", ["-n", "5"], False, True),
    ("n2_tie", ["-n", "2"], True, False),
]


def run_reference(prog, case, workdir):
    r = subprocess.run([prog] + case["args"] + ["-o", case["prefix"], case["contigs"], case["lib"]], cwd=workdir, capture_output=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for kind in FR.OUTPUTS:
        name = "%s.%s" % (case["prefix"], kind)
        got[name] = open(os.path.join(workdir, name), "rb").read()
        os.remove(os.path.join(workdir, name))
    got["stderr.txt"] = LR.strip_run_time(r.stderr.decode("latin-1")).encode("latin-1")
    return got


def checks(case, P, seqs, got, res, tie, big):
    """what the case is there to pin shows in the program's own output"""
    text = {k.split(".", 1)[1] if k != "stderr.txt" else k: v.decode("latin-1") for k, v in got.items()}
    pos, err, allf = text["contig_R.pos.tab"], text["stderr.txt"], text["contig_R.links.all"]
    seq = text["contig_R.seq.fa"]
    c = res["counters"]
    assert min(c["FR"], c["RF"], c["FF"], c["RR"]) > 0 and c["wrong"] == 2 and "Wrong_link_num: 2\n" in err, c
    assert c["repeat"] >= 2 and text["contig_R.repeat.seq.fa"], c
    assert "files number: 2\n" in err
    st = res["stats"]
    assert st[(0, 1)][:4] == (12, 5, 6, 0) and st[(3, 4)][0] == -8 and st[(2, 3)][0] == 0
    assert st[(5, 6)][:3] == (10, 3, 6)                                     # the mode tie
    assert st[(14, 15)][:3] == (9, 6, 7)                                    # conflicting and wrong records pooled
    assert st[(9, 10)][0] == -(SHORT + 6)
    rows = {int(l.split("\t")[0]): l.rstrip("\n").split("\t") for l in allf.splitlines()[1:]}
    if P.n <= 3:
        assert re.search(r"\t0\.\d{9}\n", pos)                                  # a float text of nine digits
        assert "\tctg_19\t" in pos and "\t%d\tF\n\tgap\t" % SHORT in pos      # contig 9 kept whole in front of its overlap
        assert "GGATGAC" in seq                                               # the column tie went to A
        assert "ACgTN" in seq and "ANNA" in seq
        assert ("\t5\t6\t0\t1\n" in pos)                                     # identity 1
        assert any(t.split(",")[:2] == ["31", "4"] for t in rows[29][3:]), rows[29]   # 14+ -> 15+: four records, not six
    lay = [it for items in res["layout"] for it in items if it[0] == "gap" and it[1] > 0]
    assert any(float(it[6]) < 1 for it in lay) or P.n > 4
    if big:
        assert any(t.split(",")[:3] == ["59", "1023", "3069"] for t in rows[57][3:]), rows[57]
        assert st[(28, 29)][:3] == (3, 1040, 1070)
    lengths = [sum(FR.item_len(it) for it in items) for items in res["layout"]]
    assert (len(set(lengths)) < len(lengths)) == tie, (case["name"], "ties")
    twice = [r for r in res["reads_twice"]]
    assert len(twice) == 2 and twice[0] != twice[1]


def main():
    prog = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    usage = subprocess.run([prog, "-h"], capture_output=True).stdout
    assert usage == subprocess.run([prog], capture_output=True).stdout and usage
    open(os.path.join(HERE, "fill_usage.txt"), "wb").write(usage)
    cases = []
    for n, (name, args, tie, big) in enumerate(CASES):
        rng = np.random.default_rng(500 + n)
        case = {"name": name, "args": args, "prefix": "res_" + name, "contigs": "contigs.fa", "lib": "reads.lib", "tie": tie}
        P = FR.case_params(case)
        seqs = make_contigs(rng, tie)
        S = scenario(seqs, rng, big)
        d = os.path.join(WORK, name)
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        open(os.path.join(d, "contigs.fa"), "w").write(fasta(seqs))
        cut = len(S.lines) // 3
        header = "#read_id\tread_length\t...\n"
        parts = [(S.lines[:cut], S.reads[:cut]), (S.lines[cut:], S.reads[cut:])]
        twice = [q for nm, q in S.reads if nm == "read_twice"][0]
        wrong = twice.replace("TTTTTTT", "GGGGGGG")
        parts[0][1].append(("read_twice", wrong))      # file 1 holds the id with other gap bytes; file 2's entry replaces it
        for k, (lines, reads) in enumerate(parts):
            f = "part%d.map_reads.2ctg.gz" % (k + 1)
            write_gz(os.path.join(d, f), (header + "\n".join(lines) + "\n").encode())
            write_gz(os.path.join(d, f + ".reads.fa.gz"), "".join(">%s\n%s\n" % r for r in reads).encode("latin-1"))
        open(os.path.join(d, "reads.lib"), "w").write("# the map files of this library\n\npart1.map_reads.2ctg.gz\tignored words\n"
                                                      "#skipped.gz\n  part2.map_reads.2ctg.gz\n")
        got = run_reference(prog, case, d)
        e = os.path.join(d, "expected")
        os.makedirs(e)
        for f, data in got.items():
            open(os.path.join(e, f), "wb").write(data)
        pack(case)
        want = LR.expected_outputs(OUT, case)
        mine, res = FR.run_case(OUT, case)
        assert sorted(mine) == sorted(want), (name, sorted(mine), sorted(want))
        for f in want:
            assert mine[f] == want[f], (name, f)
        res["reads_twice"] = [wrong, twice]
        assert any(nm == "read_twice" for nm, _ in parts[1][1])
        assert ("TTTTTTT" in got["res_%s.contig_R.seq.fa" % name].decode()) == (P.n <= 1)   # the one read of 22+ -> 23+ is the later entry
        checks(case, P, seqs, got, res, tie, big)
        assert os.path.getsize(os.path.join(OUT, name + ".zip")) <= 200 * 1024
        cases.append(case)
        print(name, res["counters"], os.path.getsize(os.path.join(OUT, name + ".zip")))
    open(os.path.join(OUT, "cases.json"), "w").write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    shutil.rmtree(WORK)


if __name__ == "__main__":
    main()
