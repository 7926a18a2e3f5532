"""Generate the golden vectors of the LINK / FILL edge scenarios (tests/scaffold_edge_cases.py) with the REAL reference programs.
tests/golden/scaffold_edges/ holds cases.json (per case: program, options, output prefix, contig file or lengths file, library
file) and per case one archive <case>.zip written as tests/golden/make_fill_golden.py and make_link_golden.py write theirs: fixed
dates, gz with mtime=0, expected/ with the reference's output files under their own names and stderr.txt without the `Run time:`
lines.  The fixtures are data; this script needs the reference only when it is run:

    python tests/golden/make_scaffold_edges_golden.py /path/to/link_scaffold /path/to/link_contig

The golden subset: for link_contig the scenarios column_ties and host_path_late whole, widths_x_spans cut to the widths (63, 64,
65, 129, 200) x the spans (3, 64, 65), gapstat_runs cut to the runs of up to 33 records plus one of 1024; for link_scaffold
filter_edges as one case per (-m, -i), cap_across_batches and first_seen_order.  The last two are stored as the E. coli cases of
make_link_golden.py are: contig names and lengths, and the four outputs that depend on lengths only (the program is run on
placeholder sequences of those lengths; cap_across_batches needs contigs of 3 Mb for -i 3000000).

What would take the reference into undefined behaviour is no golden: a signed 32-bit overflow in a gap or a variance, a slice
outside its read, more than 255 links on a node.

The maker asserts that the records the reference's input parses to ARE the scenario's records, and that both restatements (the
vectorised ones of tests/link_restatement.py and tests/fill_restatement.py, and the naive record-by-record ones of
tests/scaffold_edge_cases.py) reproduce every stored file or, for the naive ones, the table and the statistics behind it."""
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
sys.path.insert(0, HERE)
import fill_restatement as FR  # noqa: E402
import link_restatement as LR  # noqa: E402
import scaffold_edge_cases as E  # noqa: E402
from make_fill_golden import write_gz  # noqa: E402

OUT = os.path.join(HERE, "scaffold_edges")
LIMIT = 200 * 1024
LENGTHS_ONLY = ("scaffold.links.all", "scaffold.links.uniq", "scaffold.pos.tab", "scaffold_repeat.pos.tab")
HEADER = "#read_id\tread_length\t...\n"


def pack(src, case):
    path = os.path.join(OUT, case["name"] + ".zip")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for root, _, files in sorted(os.walk(src)):
            for f in sorted(files):
                info = zipfile.ZipInfo(os.path.relpath(os.path.join(root, f), src), date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                z.writestr(info, open(os.path.join(root, f), "rb").read())
    assert os.path.getsize(path) <= LIMIT, (case["name"], os.path.getsize(path))
    return os.path.getsize(path)


def contig_fasta(lens, seed):
    rng = np.random.default_rng(seed)
    return "".join(">ctg_%d\n%s\n" % (2 * c + 1, E.rand_bytes(rng, n)) for c, n in enumerate(lens))


def fill_lines(f):
    """the 2ctg line map_reads writes for every record: link_contig takes fields 0, 1, 3, 4, 8, 12, 14 and 18 of it"""
    out = []
    for k, (read, n, a1e, a2s, c1, c2, d1, d2, _) in enumerate(f.recs.tolist()):
        row = lambda rs, re, c, d: "read_%d\t%d\t%d\t%d\tctg_%d\t%d\t%d\t%d\t%s\t%s%%" % (  # noqa: E731
            read, n, rs, re, 2 * c + 1, f.lens[c], 1, max(re - rs + 1, 1), chr(d), "100" if k % 3 else "98.5")
        out.append(row(1, a1e, c1, d1) + "\t" + row(a2s, n, c2, d2))
    return out


def run(prog, args, workdir, names):
    r = subprocess.run([prog] + args, cwd=workdir, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {n: open(os.path.join(workdir, n), "rb").read() for n in names}
    got["stderr.txt"] = LR.strip_run_time(r.stderr.decode("latin-1")).encode("latin-1")
    return got


def store(d, got):
    os.makedirs(os.path.join(d, "expected"))
    for name, data in got.items():
        open(os.path.join(d, "expected", name), "wb").write(data)


def same_table(a, b, what):
    assert np.array_equal(np.asarray(a[0], dtype=np.int64), np.asarray(b[0], dtype=np.int64)), (what, "first")
    for f in ("target", "freq", "size"):
        assert np.array_equal(a[1][f], b[1][f]), (what, f)
    assert dict(a[2]) == dict(b[2]), (what, a[2], b[2])


def fill_case(prog, f, work):
    case = {"name": f.name, "program": "link_contig", "args": ["-n", str(f.n)], "prefix": "res_" + f.name, "contigs": "contigs.fa",
            "lib": "reads.lib", "tie": False}
    d = os.path.join(work, f.name)
    os.makedirs(d)
    open(os.path.join(d, "contigs.fa"), "w").write(contig_fasta(f.lens, len(f.recs)))
    lines = fill_lines(f)
    reads = [(int(r), f.reads[int(r)]) for r in f.recs["read"]]
    files = []
    for k, (a, b) in enumerate(zip(f.cuts[:-1], f.cuts[1:])):      # one map file per batch of the scenario
        if a == b:
            continue
        name = "part%d.map_reads.2ctg.gz" % (k + 1)
        files.append(name)
        write_gz(os.path.join(d, name), (HEADER + "\n".join(lines[a:b]) + "\n").encode())
        write_gz(os.path.join(d, name + ".reads.fa.gz"), "".join(">read_%d\n%s\n" % r for r in reads[a:b]).encode("latin-1"))
    open(os.path.join(d, "reads.lib"), "w").write("".join(x + "\n" for x in files))
    names = ["%s.%s" % (case["prefix"], k) for k in FR.OUTPUTS]
    with tempfile.TemporaryDirectory() as tmp:
        for x in os.listdir(d):
            shutil.copy(os.path.join(d, x), tmp)
        got = run(prog, case["args"] + ["-o", case["prefix"], "contigs.fa", "reads.lib"], tmp, names)
    store(d, got)
    size = pack(d, case)
    check_fill(case, f)
    return case, size


def check_fill(case, f):
    """the stored input parses to the scenario's records and reads; the restatement reproduces every stored file; the naive gap
    statistics equal the restatement's"""
    P, names, seqs, recs, files, reads = FR.load_case(OUT, case)
    assert P.n == f.n and [len(s) for s in seqs] == list(f.lens) and reads == list(f.reads), case["name"]
    assert np.array_equal(np.concatenate(recs), f.recs), case["name"]
    want = LR.expected_outputs(OUT, case)
    got, res = FR.run_case(OUT, case)
    assert len(want) == 7
    FR.compare_outputs(case, got, want)
    assert {k: v[:4] for k, v in res["stats"].items()} == E.naive_gap_stats(f.recs), case["name"]
    return res


def link_case(prog, s, work):
    lengths_only = not s.name.startswith("filter_edges")
    case = {"name": s.name, "program": "link_scaffold", "args": ["-m", str(s.P.m), "-n", str(s.P.n), "-i", str(s.P.i)],
            "prefix": "res_" + s.name, "lib": "pairs.lib", "tie": False}
    d = os.path.join(work, s.name)
    os.makedirs(d)
    lines = s.expect["lines"]
    files = []
    for k, (a, b) in enumerate(zip(s.cuts[:-1], s.cuts[1:])):
        name = "part%d.2ctg.gz" % (k + 1)
        files.append(name)
        write_gz(os.path.join(d, name), (HEADER + "\n".join(lines[a:b]) + "\n").encode())
    open(os.path.join(d, "pairs.lib"), "w").write("".join(x + "\n" for x in files))
    kinds = LENGTHS_ONLY if lengths_only else LR.OUTPUTS
    names = [LR.output_name(case, s.P, k) for k in kinds]
    with tempfile.TemporaryDirectory() as tmp:
        for x in os.listdir(d):
            shutil.copy(os.path.join(d, x), tmp)
        if lengths_only:
            case["lengths"] = "contigs.len"
            open(os.path.join(d, "contigs.len"), "w").write("".join("ctg_%d\t%d\n" % (2 * c + 1, n) for c, n in enumerate(s.lens)))
            with open(os.path.join(tmp, "contigs.fa"), "w") as fa:
                for c, n in enumerate(s.lens):
                    fa.write(">ctg_%d\n%s\n" % (2 * c + 1, "A" * n))
        else:
            case["contigs"] = "contigs.fa"
            open(os.path.join(d, "contigs.fa"), "w").write(contig_fasta(s.lens, len(lines)))
            shutil.copy(os.path.join(d, "contigs.fa"), tmp)
        got = run(prog, case["args"] + ["-o", case["prefix"], "contigs.fa", "pairs.lib"], tmp, names)
    store(d, got)
    size = pack(d, case)
    check_link(case, s)
    return case, size


def check_link(case, s):
    """the stored input parses to the scenario's records; the restatement reproduces every stored file; the naive table equals
    the restatement's"""
    P, names, lens, seqs, recs, files = LR.load_case(OUT, case)
    assert P == s.P and list(lens) == list(s.lens), case["name"]
    assert [len(r) for r in recs] == list(np.diff(s.cuts)) and np.array_equal(np.concatenate(recs), s.recs), case["name"]
    want = LR.expected_outputs(OUT, case)
    got, res = LR.run_case(OUT, case)
    assert sorted(got) == sorted(want) and len(want) == (5 if "lengths" in case else 7), (case["name"], sorted(got), sorted(want))
    for f in want:
        assert got[f] == want[f], (case["name"], f)
    same_table(E.naive_link_table(s.P, s.lens, s.recs), LR.build_table(s.P, s.lens, s.recs), case["name"])
    return res


def main():
    link_prog, fill_prog = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    work = tempfile.mkdtemp()
    cases = []
    for f in E.fill_golden_scenarios():
        case, size = fill_case(fill_prog, f, work)
        cases.append(case)
        print(case["name"], len(f.recs), size)
    for s in E.link_scenarios():
        case, size = link_case(link_prog, s, work)
        cases.append(case)
        print(case["name"], len(s.recs), size)
    open(os.path.join(OUT, "cases.json"), "w").write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
