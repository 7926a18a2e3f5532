"""Generate the link_supertig golden vectors with the REAL reference program.  tests/golden/super_cases/ holds cases.json (per
case: options, output prefix, contig file, library file) and per case one archive <case>.zip (written with fixed dates) with the
inputs (contig FASTA, the .lib file, the 2ctg map files and their .reads.fa.gz as gz written with mtime=0) and expected/ with
everything the reference wrote: its seven output files under their own names and stderr.txt without the `Run time:` lines.
super_usage.txt is the usage text (the program writes it to stderr).  The fixtures are data; this script needs the reference only
when it is run:

    python tests/golden/make_super_golden.py /path/to/link_supertig

The program is the x86-64 binary the reference ships as link_scaffold/link_supertig (or one built by link_scaffold/Makefile; it
needs Boost).  The fixtures here were written by the shipped binary.

The inputs are what map_reads writes for long reads laid over the junctions of oriented contigs.  Every spanning read is present
and has at least 250 bases in front of the middle of its gap, so the reference's substr stays inside its read and the program
exits 0 (asserted).  Every case is asserted to show what it is meant to pin (see checks()), and tests/super_restatement.py to
equal the program on every case."""
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
import super_restatement as SR  # noqa: E402

OUT = os.path.join(HERE, "super_cases")
N_CONTIGS = 23
SHORT = 300                                            # the contig the interleaving pass steps over
ODD_BYTES = "acgtnNRYxACGTACGTACGTACGTA"               # gap bytes with lower case, n, N and other letters
BIG = [3] * 1040 + [4] * 30                            # a pair of more than 1023 records


def pack(work, case):
    d = os.path.join(work, case["name"])
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
    """long reads laid over the junction of two oriented contigs, and the 2ctg line map_reads writes for each"""

    def __init__(self, seqs, rng):
        self.seqs, self.rng, self.lines, self.reads, self.n = seqs, rng, [], [], 0

    def oriented(self, c, o):
        return self.seqs[c] if o == "+" else LR.reverse_complement(self.seqs[c])

    def read(self, X, ox, Y, oy, gap, filler=None, reverse=False, d1=None, d2=None, la=400, lb=400, seq_of=None, raw=False):
        """one read: the last la bases of X(ox), gap filler bytes, the first lb bases of Y(oy); reverse: the read is the other
        strand, so its first alignment lies on Y.  d1 / d2 override the direction fields; raw: a read of the other strand holds the filler bytes
        as they are, not their reverse complement; seq_of: a read made earlier whose
        sequence and line geometry this one repeats under a new name."""
        self.n += 1
        name = "read_%d" % self.n
        left, right = self.oriented(X, ox), self.oriented(Y, oy)
        la, lb = min(la, len(left)), min(lb, len(right))
        if filler is None:
            filler = rand_seq(self.rng, max(gap, 0))
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
            # the read now begins with what follows Y's part: alignment 1 is Y's, it ends at e1; alignment 2 (X's) begins gap + 1 behind
            e1 = n - (la + max(gap, 0) + lb) + lb
            s2 = e1 + gap + 1
            if raw:
                seq = seq[:e1] + filler + seq[e1 + gap:]
            X, ox, Y, oy, la, lb = Y, flip[oy], X, flip[ox], lb, la
        if seq_of is not None:
            seq = seq_of
        D = {"+": "F", "-": "R"}
        d1, d2 = d1 or D[ox], d2 or D[oy]
        row = lambda rs, re, c, d: "%s\t%d\t%d\t%d\tctg_%d\t%d\t%d\t%d\t%s\t%s%%" % (  # noqa: E731
            name, n, rs, re, 2 * c + 1, len(self.seqs[c]), 1, max(re - rs + 1, 1), d, "100" if self.n % 3 else "98.5")
        self.lines.append(row(max(e1 - la + 1, 1), e1, X, d1) + "\t" + row(s2, min(s2 + lb - 1, n), Y, d2))
        self.reads.append((name, seq))
        return seq

    def junction(self, X, ox, Y, oy, gaps, filler=None, **kw):
        """reads over X(ox) -> Y(oy) with the given gaps, alternately of either strand, every read with gap bytes of its own"""
        for k, g in enumerate(gaps):
            self.read(X, ox, Y, oy, g, filler, reverse=k % 2 == 1, **kw)


def make_contigs(rng, tie):
    lens = [int(x) for x in rng.choice(np.arange(700, 1300), N_CONTIGS, replace=False)]
    lens[9] = SHORT
    if tie:
        lens[22] = lens[21]                            # two one-contig super-contigs of one length
    return [rand_seq(rng, n) for n in lens]


def fasta(seqs):
    out = []
    for c, s in enumerate(seqs):
        out.append(">ctg_%d%s\n" % (2 * c + 1, "  length:%d" % len(s) if c % 3 == 0 else ""))
        width = 60 if c % 4 == 1 else len(s)
        out += [s[p:p + width] + "\n" for p in range(0, len(s), width)]
    return "".join(out)


def scenario(seqs, rng, big):
    S = Scenario(seqs, rng)
    # (a) a chain 0+ 1+ 2- 3+ 4+ 5+
    S.junction(0, "+", 1, "+", [120, 120, 120, 121, 119, 120])
    #     more than 16 slices, several of one length with different bytes: the introsort path of the reference's sort
    S.junction(1, "+", 2, "-", [60, 60, 61, 63, 60, 59] * 3 + [60, 61])
    #     an odd gap
    S.junction(2, "-", 3, "+", [15, 15, 15, 15, 17])
    #     slices clamped by the end of their read: 550 and 451 bytes are written, 450 (= 0.75 x 600 exactly) and 449 are not
    S.junction(3, "+", 4, "+", [100] * 5)
    for lb in (100, 200, 99, 101):
        S.read(3, "+", 4, "+", 100, lb=lb)
    #     overlaps whose sum is odd and negative: -11 / 3 is -3 in C, slices of 500 bytes, N x 1
    S.junction(4, "+", 5, "+", [-3, -4, -4])
    # (b) slices that begin at the first byte of their read
    S.junction(6, "+", 7, "+", [40] * 4, la=250, lb=250)
    # (c) 8 -> 9 -> 10 with 9 short and 8 -> 10 over it: the interleaving pass removes 8 -> 10
    S.junction(8, "+", 9, "+", [50] * 5)
    S.junction(9, "+", 10, "+", [50] * 5)
    S.junction(8, "+", 10, "+", [50 + SHORT + 50] * 5)
    # (d) a node with two incoming links: a repeat contig
    S.junction(11, "+", 13, "+", [30] * 5)
    S.junction(12, "+", 13, "+", [45] * 5)
    # (e) links of 2 and 4 records: cut by -n 3 / -n 5
    S.junction(14, "+", 15, "+", [20, 20])
    S.junction(15, "+", 16, "-", [10] * 4)
    # (f) lower case, n, N and other bytes in the slices of a gap, half of them reversed
    S.junction(17, "+", 18, "-", [len(ODD_BYTES)] * 5, filler=ODD_BYTES, raw=True)
    # (g) a wrong direction: in the statistics and in the slices, not in the links
    S.read(0, "+", 1, "+", 130, d1="N")
    if big:
        # (h) a link of more than 1023 records: the link stops counting, the statistics do not.  Four read sequences per gap size.
        made = {}
        for k, g in enumerate(BIG):
            key = (g, k % 4)
            made[key] = S.read(19, "+", 20, "+", g, reverse=k % 2 == 1, la=260, lb=260, seq_of=made.get(key))
    return S


CASES = [  # name, args, tie, big
    ("n_default", [], False, True),
    ("n1", ["-n", "1"], False, False),
    ("n5", ["-n", "5"], False, False),
    ("n2_tie", ["-n", "2"], True, False),
]


def run_reference(prog, case, workdir):
    r = subprocess.run([prog] + case["args"] + ["-o", case["prefix"], case["contigs"], case["lib"]], cwd=workdir, capture_output=True,
                       timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = {}
    for kind in SR.OUTPUTS:
        name = "%s.%s" % (case["prefix"], kind)
        got[name] = open(os.path.join(workdir, name), "rb").read()
        os.remove(os.path.join(workdir, name))
    got["stderr.txt"] = LR.strip_run_time(r.stderr.decode("latin-1")).encode("latin-1")
    return got


def checks(case, P, got, res, tie, big):
    """what the case is there to pin shows in the program's own output"""
    text = {k.split(".", 1)[1] if k != "stderr.txt" else k: v.decode("latin-1") for k, v in got.items()}
    pos, err, allf, gap = text["supertig.pos.tab"], text["stderr.txt"], text["supertig.links.all"], text["supertig.gap.data"]
    c = res["counters"]
    assert min(c["FR"], c["RF"], c["FF"], c["RR"]) > 0 and c["wrong"] == 1 and "Wrong_link_num: 1\n" in err, c
    assert "files number: 2\n" in err
    st = res["stats"]
    assert st[(0, 1)][:5] == (121, 119, 130, 7, 2)                            # the wrong-direction line counts
    assert st[(4, 5)][:5] == (-3, -4, -3, 3, 0)                               # -11 / 3 truncates toward zero
    assert st[(2, 3)][:4] == (15, 15, 17, 5)
    rows = {int(l.split("\t")[0]): l.rstrip("\n").split("\t") for l in allf.splitlines()[1:]}
    assert any(t.split(",")[:2] == ["3", "6"] for t in rows[1][3:]), rows[1]  # 0+ -> 1+: six records, not seven
    J = {(j["left"], j["right"]): j for j in res["junctions"]}
    if P.n <= 3:
        assert c["interleave"] == 2 and "Removed interleave links num: 2\n" in err
        assert c["repeat"] == 1 and text["supertig_repeat.seq.fa"]
        assert "\t-4\t-3\t3\t0\n" in pos and "Error may happens: mean_gap_size <= 0\n" in err
        j = J[(4, 5)]
        assert j["written"] == 1 and all(s[0] == 500 for s in j["slices"])  # overlaps: slices of 500 bytes
        j = J[(1, 2)]
        lengths = [s[0] for s in j["slices"]]
        assert len(lengths) == 20 and lengths.count(560) >= 8 and len({s[4] for s in j["slices"] if s[0] == 560}) >= 8
        assert "N\t59\t63\t20\t" in pos
        j = J[(3, 4)]
        assert sorted(s[0] for s in j["slices"]) == [449, 450, 451, 550] + [600] * 5
        assert sorted(s[0] for s in j["slices"] if not s[3]) == [449, 450]
        g = j["gap_id"]
        assert "Altert message:  gap_id %d  600\t450\n" % g in err and "Altert message:  gap_id %d  600\t449\n" % g in err
        j = J[(6, 7)]
        assert all(s[0] == 540 for s in j["slices"])
        j = J[(17, 18)]
        assert any(s[2] and "nNRYx" not in s[4] and "N" in s[4] for s in j["slices"]) and any(not s[2] and ODD_BYTES in s[4] for s in j["slices"])
        assert ODD_BYTES in gap and LR.reverse_complement(ODD_BYTES) in gap
        assert (8, 9) in J and (9, 10) in J and (8, 10) not in J
        assert any(it[0] == "ctg" and it[2] for its in res["layout"] for it in its)
    if big:
        assert any(t.split(",")[:3] == ["41", "1023", "3069"] for t in rows[39][3:]), rows[39]
        assert st[(19, 20)][:5] == (3, 3, 4, 1070, 0)
        assert len(J[(19, 20)]["slices"]) == 1070
    lengths = [sum(SR.item_len(it) for it in items) for items in res["layout"]]
    assert (len(set(lengths)) < len(lengths)) == tie, (case["name"], "ties")


def pos_zero(recs, reads):
    """records whose slice begins at byte 0 of its read"""
    n = 0
    for r in recs:
        geo = SR.slice_geometry(int(r["align1_end"]), int(r["align2_start"]), len(reads[int(r["read"])]))
        assert geo is not None
        n += geo[0] == 0
    return n


def main():
    prog = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    work = tempfile.mkdtemp()
    u = subprocess.run([prog, "-h"], capture_output=True)
    assert u.returncode == 0 and u.stderr and not u.stdout
    for args in ([], ["only_one_argument"]):
        v = subprocess.run([prog] + args, capture_output=True)
        assert v.returncode == 0 and v.stderr == u.stderr
    assert subprocess.run([prog, "-n", "5", "-h"], capture_output=True).stderr == u.stderr.replace(b"default=3", b"default=5")
    assert u.stderr.decode() == SR.usage_text()
    open(os.path.join(HERE, "super_usage.txt"), "wb").write(u.stderr)
    cases = []
    for n, (name, args, tie, big) in enumerate(CASES):
        rng = np.random.default_rng(900 + n)
        case = {"name": name, "args": args, "prefix": "res_" + name, "contigs": "contigs.fa", "lib": "reads.lib", "tie": tie}
        P = SR.case_params(case)
        seqs = make_contigs(rng, tie)
        S = scenario(seqs, rng, big)
        d = os.path.join(work, name)
        os.makedirs(d)
        open(os.path.join(d, "contigs.fa"), "w").write(fasta(seqs))
        cut = 16                                       # the records of 1+ -> 2- lie in both files: file order decides among equal lengths
        header = "#read_id\tread_length\t...\n"
        parts = [(S.lines[:cut], S.reads[:cut]), (S.lines[cut:], S.reads[cut:])]
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
        pack(work, case)
        want = LR.expected_outputs(OUT, case)
        mine, res = SR.run_case(OUT, case)
        assert sorted(mine) == sorted(want) and len(want) == 8, (name, sorted(mine), sorted(want))
        for f in want:
            assert mine[f] == want[f], (name, f)
        _, _, _, recs, _, reads = SR.load_case(OUT, case)
        assert len(recs[0]) == cut and pos_zero(np.concatenate(recs), reads) >= 4
        checks(case, P, got, res, tie, big)
        assert os.path.getsize(os.path.join(OUT, name + ".zip")) <= 200 * 1024
        cases.append(case)
        print(name, res["counters"], os.path.getsize(os.path.join(OUT, name + ".zip")))
    open(os.path.join(OUT, "cases.json"), "w").write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
