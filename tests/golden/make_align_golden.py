#!/usr/bin/env python3
"""Writes tests/golden/align_cases/: what the REAL reference computes for the alignments of the bubbles pass.

pairs.npz    a few hundred string pairs with the aligned strings and the score the reference's global_aligning()
             (DBG_contig/global_aligning.cpp) returned for each.  The reference's global_aligning.cpp is compiled where it lies into a
             scratch directory, behind a small driver of this project's own (DRIVER below: it declares the function, reads pairs from
             stdin and prints what came back).  Lengths: (1,1), (1,5), (5,1), (63,64), (64,64), (65,63), (64,129), (128,128), (129,131),
             (163,164) and both sides of DBGK_ALIGN_MAX_LEN; pairs above the bound carry no expected alignment.  Content: random over ACGT,
             over two letters and over one letter (where the tie rule of get_max_score decides nearly every cell), identical strings,
             strings without a common letter, one string a prefix, a suffix or an infix of the other, a string and a copy of it with a few
             substitutions and one indel, and the composed arms of contig_cases/d_bubbles.
<case>.npz   inputs for bin/debruijn_contig in the format of tests/golden/contig_cases, each with what the real reference program wrote at
             -t 1 (built as tests/golden/make_contig_golden.py builds it):
  a_indel_lengths          indel bubbles whose arm lengths differ by 1, 5, 9 and 10: with -U 100 -L 0.1 the one of 9 is removed, the one of
                           10 is kept
  b_equal_length_aligned   equal-length arms that are aligned: a base deleted and one inserted 8 further on (type INDEL with equal lengths,
                           removed), five substitutions in 41 (above -E, aligned, kept); and four in 40, which is not above 0.1 and takes
                           the SNP branch
  c_indel_after_bubble     an indel bubble whose branch node an earlier removal of the pass creates (the layout of
                           simplify_cases/e_bubble_after_bubble): it has no submitted pair and is aligned on the host; a second indel
                           bubble far from it is aligned on the GPU
check() asserts on the restated pass (tests/align_restatement.py) that each case shows what its name says.

No case shows a submitted pair whose strings an earlier removal of the pass has changed, and none can: see NO_STALE_PAIR below.

    python tests/golden/make_align_golden.py --ref DIR [--scratch DIR]
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import align_restatement as A  # noqa: E402
import contig_restatement as R  # noqa: E402
import simplify_restatement as S  # noqa: E402
from make_contig_golden import COMP, SUFFIXES, build_reference, rand_seq, sample_reads  # noqa: E402

NO_STALE_PAIR = """A pair is submitted for a list entry Y whose two arms are traced and end on one node L.  The bubbles pass changes a node in
two ways only: it deletes the nodes of a removed arm, and it recalculates that arm's last node and its branch node.  A removed arm is a
whole chain of linear nodes between two nodes that are not linear, so if it shares a node with an arm of Y it is that arm, removed from
the entry at its other end, and then Y has one edge left there and is no bubble any more: nothing is aligned.  L stays a node with two
edges on one side as long as both arms run into it, and Y's own two edges are what makes it an entry.  So when the loop reaches an
entry that submitted a pair and still finds a bubble there, it holds the strings it submitted.  The comparison of the strings is kept
as the whole validity rule all the same (it costs O(L)); tests reach its other branch through the hook align_stale=1, which submits every
pair with its two strings exchanged."""

MAX_LEN = A.MAX_LEN
LENGTHS = [(1, 1), (1, 5), (5, 1), (63, 64), (64, 64), (65, 63), (64, 129), (128, 128), (129, 131), (163, 164), (MAX_LEN - 1, MAX_LEN),
           (MAX_LEN, MAX_LEN), (MAX_LEN, 1), (1, MAX_LEN)]
OVER = [(MAX_LEN + 1, MAX_LEN), (MAX_LEN, MAX_LEN + 1), (MAX_LEN + 1, MAX_LEN + 1), (300, 10)]

DRIVER = r"""
// reads "seq_i seq_j" per line, prints "score align_i align_j" as the linked global_aligning() returns them
#include <iostream>
#include <string>
void global_aligning(std::string &seq_i, std::string &seq_j, std::string &align_i, std::string &align_j, int &final_score);
int main()
{
	std::string a, b;
	while (std::cin >> a >> b) {
		std::string x, y;
		int score = 0;
		global_aligning(a, b, x, y, score);
		std::cout << score << " " << x << " " << y << "\n";
	}
	return 0;
}
"""


def build_driver(ref, scratch):
    src, exe = os.path.join(scratch, "align_driver.cpp"), os.path.join(scratch, "align_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["g++", "-O2", "-w", "-std=c++17", "-I", ref, "-o", exe, src, os.path.join(ref, "global_aligning.cpp")], check=True)
    return exe


def mutated(rng, s, n_out):
    """a copy of s with a few substitutions, brought to n_out letters by one deletion or one insertion"""
    r = list(s)
    for _ in range(max(1, len(r) // 30)):
        p = rng.randrange(len(r))
        r[p] = rng.choice([c for c in "ACGT" if c != r[p]])
    if n_out < len(r):
        p = rng.randrange(len(r) - n_out + 1)
        r = r[:p] + r[p + len(r) - n_out:]
    elif n_out > len(r):
        p = rng.randrange(len(r) + 1)
        r = r[:p] + list(rand_seq(rng, n_out - len(r))) + r[p:]
    return "".join(r)


def letters(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def pair_list(d_bubbles_arms):
    rng = random.Random(2601)
    pairs = []
    for li, lj in LENGTHS:
        for _ in range(4):
            pairs.append((rand_seq(rng, li), rand_seq(rng, lj)))
        for _ in range(4):
            two = "".join(rng.sample("ACGT", 2))
            pairs.append((letters(rng, li, two), letters(rng, lj, two)))
        one = rng.choice("ACGT")
        pairs.append((one * li, one * lj))
        s = rand_seq(rng, li)
        pairs.append((s, s))                                             # identical
        pairs.append((letters(rng, li, "AC"), letters(rng, lj, "GT")))   # no common letter
        long_one = rand_seq(rng, max(li, lj))
        short = min(li, lj)
        for cut in (long_one[:short], long_one[len(long_one) - short:], long_one[(len(long_one) - short) // 2:][:short]):   # prefix, suffix, infix
            pairs.append((long_one, cut) if li >= lj else (cut, long_one))
        s = rand_seq(rng, li)
        pairs.append((s, mutated(rng, s, lj)))
    pairs += d_bubbles_arms
    for li, lj in OVER:
        pairs.append((rand_seq(rng, li), rand_seq(rng, lj)))
    return pairs


def d_bubbles_arms():
    c = R.load_case(os.path.join(HERE, "contig_cases", "d_bubbles.npz"))
    o = R.Options.from_args(c["args"])
    t = R.Table.from_case(c)
    tips, branches, _, _ = R.first_pass(t, o)
    err = []
    S.remove_tips(t, o, tips, err)
    S.remove_low_edges(t, o, branches, err)
    every = []
    A.collect(S.Pass(t, o), o, branches, every=every)
    assert len(every) >= 4 and any(n1 != n2 for _, _, _, n1, n2 in every)
    return [(s1, s2) for _, s1, s2, _, _ in every]


def write_pairs(ref, scratch, out_root):
    pairs = pair_list(d_bubbles_arms())
    fits = [max(len(a), len(b)) <= MAX_LEN for a, b in pairs]
    exe = build_driver(ref, scratch)
    text = "".join("%s %s\n" % (a, b) for (a, b), f in zip(pairs, fits) if f)
    p = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True)
    answers = iter(p.stdout.decode().split("\n"))
    score, a_i, a_j = [], [], []
    for (a, b), f in zip(pairs, fits):
        if f:
            sc, x, y = next(answers).split(" ")
            assert x.replace("-", "") == a and y.replace("-", "") == b and len(x) == len(y)
        else:
            sc, x, y = 0, "", ""
        score.append(int(sc))
        a_i.append(x)
        a_j.append(y)
    blob = lambda strings: np.frombuffer("".join(strings).encode(), dtype=np.uint8)                       # noqa: E731
    offs = lambda strings: np.cumsum([0] + [len(s) for s in strings]).astype(np.uint32)                   # noqa: E731
    np.savez_compressed(os.path.join(out_root, "pairs.npz"), seq_i=blob(a for a, _ in pairs), seq_i_off=offs([a for a, _ in pairs]),
                        seq_j=blob(b for _, b in pairs), seq_j_off=offs([b for _, b in pairs]), align_i=blob(a_i), align_j=blob(a_j),
                        align_off=offs(a_i), score=np.array(score, dtype=np.int32), fits=np.array(fits, dtype=np.uint8))
    print("pairs.npz: %d pairs, %d above the bound, %d bytes" % (len(pairs), fits.count(False), os.path.getsize(os.path.join(out_root, "pairs.npz"))))


ARGS = ["-k", "31", "-D", "1", "-M", "100"]          # -U 100, -L 0.1, -E 0.1


def delete(seq, at, n):
    return seq[:at] + seq[at + n:]


def substitute(seq, places):
    s = list(seq)
    for p in places:
        s[p] = COMP[s[p]]
    return "".join(s)


def cases():
    c = {}
    rng = random.Random(2701)
    h1 = rand_seq(rng, 6000)
    h2 = h1
    for at, n in ((5000, 10), (4000, 9), (2500, 5), (1000, 1)):           # from the far end, so that the places stay where they are
        h2 = delete(h2, at, n)
    c["a_indel_lengths"] = sample_reads(rng, h1, 16) + sample_reads(rng, h2, 11)

    rng = random.Random(2802)
    h1 = rand_seq(rng, 6000)
    h2 = substitute(h1, (3000, 3003, 3005, 3008))                       # 4 in 40
    h2 = substitute(h2, (4500, 4502, 4504, 4506, 4509))                 # 5 in 41
    ins = rng.choice([b for b in "ACGT" if b != h2[1009]])
    h2 = h2[:1000] + h2[1001:1009] + ins + h2[1009:]                    # one base out at 1000, one in 8 further on
    assert len(h2) == len(h1)
    c["b_equal_length_aligned"] = sample_reads(rng, h1, 16) + sample_reads(rng, h2, 11)

    rng = random.Random(2903)
    h1 = rand_seq(rng, 3000)
    h2 = delete(h1, 2000, 3)                                            # an indel bubble of its own, far from the two
    h2 = delete(substitute(h2, (1000,)), 1032, 4)                       # k + 1 apart: exactly one k-mer lies between the two bubbles
    c["c_indel_after_bubble"] = sample_reads(rng, h1, 16) + sample_reads(rng, h2, 11)
    return c


def check(name, shows, counts, log, every, bubble_fa):
    """every case shows what its name says; log: (entry, used, len1, len2, submitted) per alignment of the pass"""
    records = [ln.split("\t") for ln in bubble_fa.decode().split("\n") if ln.startswith(">")]
    indel = [(int(r[2].split()[1]), int(r[4].split()[1])) for r in records if r[1] == "type: INDEL"]
    if name == "a_indel_lengths":
        removed = sorted(abs(a - b) for a, b in indel)
        assert removed == [1, 5, 9], removed
        assert any(abs(n1 - n2) == 10 for _, _, n1, n2, _ in log) and counts["host"] == 0 and counts["used"] >= 4, (counts, log)
    elif name == "b_equal_length_aligned":
        assert any(a == b for a, b in indel), indel                                          # type INDEL with equal lengths, removed
        assert any(n1 == n2 == 41 and used for _, used, n1, n2, _ in log), log               # above -E: aligned
        aligned_entries = {i for i, _, _, _, _ in log}
        exact = [i for i, s1, s2, n1, n2 in every if n1 == n2 == 40 and R.count_differences(s1, s2) == 4]
        assert exact and not (set(exact) & aligned_entries), (exact, log)                    # exactly 4 / 40: the SNP branch
        assert counts["host"] == 0
    elif name == "c_indel_after_bubble":
        assert any(not used and not sub and n1 != n2 for _, used, n1, n2, sub in log), log    # no pair of its own: on the host
        assert counts["host"] > 0 and shows["bubbles_indel"] > 0 and shows["bubbles_snp"] > 0
    assert counts["too_long"] == 0 and (counts["submitted"] == 0 or counts["used"] >= 1), counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's DBG_contig source directory")
    ap.add_argument("--scratch", default=None)
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="align_golden_")
    os.makedirs(scratch, exist_ok=True)
    out_root = os.path.join(HERE, "align_cases")
    os.makedirs(out_root, exist_ok=True)
    write_pairs(a.ref, scratch, out_root)
    exe = build_reference(a.ref, scratch)
    ref_dbg = os.path.join(ROOT, "oracle", "_ref", "ref_dbg")
    for name, reads in cases().items():
        args = ARGS + ["-r", "150", "-f", "2", "-i", "0.00002"]
        work = os.path.join(scratch, name)
        os.makedirs(work, exist_ok=True)
        fasta = "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)).encode()
        with open(os.path.join(work, "reads.fa"), "wb") as f:
            f.write(fasta)
        lib = os.path.join(work, "reads.lib")
        with open(lib, "w") as f:
            f.write(os.path.join(work, "reads.fa") + "\n")
        p = subprocess.run([exe] + args + ["-t", "1", "-o", os.path.join(work, "out"), lib], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        err = "\n".join(ln for ln in p.stderr.decode().split("\n") if "Run time:" not in ln).replace(work, "WORK")
        err = err[err.index("Start to calulate kmer links information!"):]     # the contig stage's part
        outputs = {s: open(os.path.join(work, "out.contig." + s), "rb").read() for s in SUFFIXES}
        img = os.path.join(work, "table.img")                                   # the reference's table, slot for slot
        graph_args = [x for pair in zip(args[::2], args[1::2]) if pair[0] in ("-k", "-r", "-f", "-i") for x in pair]
        subprocess.run([ref_dbg, "build"] + graph_args + ["-t", "1", "-T", img, "-q", lib], stdout=subprocess.PIPE, check=True)
        t = R.Table.from_image(open(img, "rb").read(), 31)
        slots = [i for i in range(t.size) if t.filled[i]]
        case = {"k": 31, "table_size": np.uint64(t.size), "slots": np.array(slots, dtype=np.uint32), "kmers": np.array([t.kmer[i] for i in slots], dtype=np.uint64),
                "l_links": np.array([t.l_link[i] for i in slots], dtype=np.uint32), "r_links": np.array([t.r_link[i] for i in slots], dtype=np.uint32)}
        o = R.Options.from_args(args)
        files, _, _ = R.run_stage(R.Table.from_case(case), o)
        res = A.run_passes(R.Table.from_case(case), o)
        shows = {
            "restatement_equal": all(outputs[s] == files.get(s) for s in SUFFIXES) and all(outputs[s] == b for s, b in res["files"].items()),
            "tips": files["tip.fa"].count(b">"), "lowedges": files["lowedge.fa"].count(b">"),
            "bubbles_snp": files["bubble.fa"].count(b"type: SNP"), "bubbles_indel": files["bubble.fa"].count(b"type: INDEL"),
            "counts": {p: list(v) for p, v in res["counts"].items()}, "aligned": res["aligned"],
        }
        as_bytes = lambda b: np.frombuffer(b, dtype=np.uint8)   # noqa: E731
        arrays = {f: case[f] for f in ("table_size", "slots", "kmers", "l_links", "r_links")}
        arrays.update(args=as_bytes(json.dumps(args).encode()), shows=as_bytes(json.dumps(shows, sort_keys=True).encode()), stderr=as_bytes(err.encode("latin-1")),
                      reads=as_bytes(fasta))
        arrays.update({"out." + s: as_bytes(b) for s, b in outputs.items()})
        np.savez_compressed(os.path.join(out_root, name + ".npz"), **arrays)
        print(name, json.dumps(shows, sort_keys=True))
        assert shows["restatement_equal"], name
        check(name, shows, res["aligned"], res["log"], res["every"], outputs["bubble.fa"])


if __name__ == "__main__":
    main()
