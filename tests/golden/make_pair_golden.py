"""Generate the pair-merge golden vectors (tests/golden/pair_cases/) with the REAL reference program run with -j 1.

Table and reads are those of tests/golden/correct_k13.  Mate file 1 is reads.fq.gz; mate file 2 holds the same 412 records rotated
by one, so that pair i is (read i, read i + 1) and every class of pair occurs: both mates kept, only mate 1, only mate 2, neither.
The reference corrects both files, merges them (merge_two_corr_files, correct_error/correct.cpp:851-922) and -- unlike this
project's program -- removes the two per-file outputs afterwards; what is stored per case is

    <case>.pair.fa.gz  <case>.single.fa.gz   the two merged files, recompressed without a time stamp
    <case>.pair.single.stat                  the four numbers

The maker asserts, from the reference's own output, the number of pairs of every class (tests/pair_restatement.py, CASES).  The
fixtures are data; this script needs the reference only when it is run.

    python tests/golden/make_pair_golden.py oracle/_ref/ref_correct
"""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import pair_restatement as PR  # noqa: E402
from make_correct_golden import write_bytes  # noqa: E402


def rotated_fq(src, dst):
    """the four-line records of src rotated by one -> dst (plain text)"""
    lines = gzip.open(src, "rb").read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    recs = [lines[i:i + 4] for i in range(0, len(lines) - 1, 4)]
    with open(dst, "wb") as f:
        f.write(b"".join(b"\n".join(r) + b"\n" for r in recs[1:] + recs[:1]))
    return len(recs)


def main():
    exe = os.path.abspath(sys.argv[1])
    os.makedirs(PR.GOLDEN, exist_ok=True)
    for name, (_, opts, want) in PR.CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            f1, f2 = os.path.join(tmp, "reads_1.fq.gz"), os.path.join(tmp, "reads_2.fq")
            shutil.copy(os.path.join(PR.CORRECT, "reads.fq.gz"), f1)
            n = rotated_fq(f1, f2)
            assert n == 412
            with open(os.path.join(tmp, "reads.lib"), "w") as f:
                f.write("%s\n%s\n" % (f1, f2))
            subprocess.run([exe, "-k", "13", "-t", "4", "-f", "1", "-j", "1"] + opts + [os.path.join(PR.CORRECT, "table.cz"), os.path.join(tmp, "reads.lib")],
                           capture_output=True, check=True, timeout=600)
            pair = gzip.open(f1 + ".correct.fa.gz.pair.fa.gz", "rb").read()
            single = gzip.open(f1 + ".correct.fa.gz.single.fa.gz", "rb").read()
            stat = open(f1 + ".correct.fa.gz.pair.single.stat", "rb").read()
        # the classes, from the reference's own output: a header names its read (r<i>/1), mate 2 of pair i is read i + 1
        p = pair.split(b"\n")[:-1]
        s = single.split(b"\n")[:-1]
        index = lambda head: int(head.split()[0][2:].split(b"/")[0])
        both = len(p) // 4
        firsts = {index(h) for h in p[0::4]}
        only1 = only2 = 0
        seen = {}
        for h in s[0::2]:
            seen[index(h)] = seen.get(index(h), 0) + 1
        # read r is mate 1 of pair r and mate 2 of pair r - 1; it is single once for every of the two whose other mate is empty
        kept = firsts | {index(h) for h in p[2::4]} | set(seen)
        for i in range(n):
            if i in firsts:
                continue
            a, b = i in kept, (i + 1) % n in kept
            only1 += a and not b
            only2 += b and not a
        got = (both, only1, only2, n - both - only1 - only2)
        assert got == want, (name, got, want)
        assert sum(seen.values()) == only1 + only2 and all(x > 0 for x in got), (name, got)
        write_bytes(os.path.join(PR.GOLDEN, name + ".pair.fa.gz"), pair, True)
        write_bytes(os.path.join(PR.GOLDEN, name + ".single.fa.gz"), single, True)
        open(os.path.join(PR.GOLDEN, name + ".pair.single.stat"), "wb").write(stat)
        print(name, got, stat.decode().split())


if __name__ == "__main__":
    main()
