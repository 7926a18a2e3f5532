#!/usr/bin/env python3
"""Writes tests/golden/contig_cases/: per case the reads, the option list, the table dump and what the REAL reference program wrote.

The reference's DBG_contig sources are compiled where they lie (REF, default /root/reference/DBG_contig) into a scratch directory
outside the repository, with -I oracle/standin for the two Boost headers and kmerSet.cpp at -O0 (see oracle/Makefile), into a
complete CPU-only debruijn_contig; it runs at -t 1.  The table dump (occupied slots: slot, kmer, l_link, r_link) comes from
oracle/_ref/ref_dbg, the reference's graph stage behind this project's driver, run with the same options.  Per case one compressed
<name>.npz (contig_restatement.load_case reads it): the reads file, the option list, the table's occupied slots, the stage's stderr
(without `Run time:` lines), the out.contig.* files and what the case shows.
Every case is checked to show what it pins, and the restatement (tests/contig_restatement.py) says for each whether the reference's
walk meets a structure the GPU read-out hands to the host walker.

    python tests/golden/make_contig_golden.py [--ref DIR] [--scratch DIR]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import contig_restatement as R  # noqa: E402

SOURCES = ["main", "kmerSet", "seqKmer", "DBGgraph", "gzstream", "contig", "global_aligning"]
SUFFIXES = ["kmer.freq", "tip.fa", "lowedge.fa", "bubble.fa", "seq.fa", "seq.depth", "small.fa", "small.depth"]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def build_reference(ref, scratch):
    exe = os.path.join(scratch, "debruijn_contig_ref")
    objs = []
    for s in SOURCES:
        o = os.path.join(scratch, s + ".o")
        subprocess.run(["g++", "-O0" if s == "kmerSet" else "-O2", "-w", "-std=c++17", "-I", os.path.join(ROOT, "oracle", "standin"), "-I", ref,
                        "-c", os.path.join(ref, s + ".cpp"), "-o", o], check=True)
        objs.append(o)
    subprocess.run(["g++", "-o", exe] + objs + ["-lz", "-lpthread"], check=True)
    return exe


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def sample_reads(rng, seq, cov, rlen=100, err=0.0, circular=False):
    """reads of rlen from either strand; the two ends of a linear sequence are sampled as often as its middle"""
    out, n = [], len(seq)
    src = seq + seq[:rlen] if circular else seq
    for _ in range(max(1, int(cov * n / rlen))):
        p = rng.randrange(n) if circular else rng.randrange(-rlen // 2, n - rlen // 2)
        p = p if circular else min(max(p, 0), n - rlen)
        r = list(src[p:p + rlen])
        for i in range(len(r)):
            if rng.random() < err:
                r[i] = rng.choice([c for c in "ACGT" if c != r[i]])
        r = "".join(r)
        out.append(r if rng.random() < 0.5 else revcomp(r))
    return out


def tile_reads(seq, times, rlen=100, step=7):
    """every window of rlen at a fixed step, and both ends, `times` each: the same depth pattern for every sequence of one length"""
    starts = sorted(set(list(range(0, len(seq) - rlen + 1, step)) + [len(seq) - rlen]))
    return [seq[p:p + rlen] for p in starts for _ in range(times)]


def cases():
    c = {}
    rng = random.Random(101)
    g = rand_seq(rng, 2400)
    rep = rand_seq(rng, 180)
    genome = g[:700] + rep + g[700:1500] + rep + g[1500:] + rep + rand_seq(rng, 300)
    c["a_repeat"] = (["-k", "31", "-M", "100"], sample_reads(rng, genome, 20))

    rng = random.Random(202)
    genome = rand_seq(rng, 3000)
    reads = sample_reads(rng, genome, 18, err=0.003)
    # a dead end longer than -I at low depth: get_linear_path stops after -I steps (contig.cpp:810), so the length test of :308 always
    # holds and the first -I nodes of it are removed as a tip of -I + k bases; no tip is kept for its length
    long_tip = genome[1000:1040] + rand_seq(rng, 110)          # one read of 150, three times
    deep_tip = genome[2500:2560] + rand_seq(rng, 25)           # a short dead end deeper than -P
    reads += [long_tip] * 3 + [deep_tip] * 7
    c["b_tips"] = (["-k", "31", "-D", "1", "-I", "100", "-P", "3", "-M", "100"], reads)

    rng = random.Random(303)
    genome = rand_seq(rng, 3000)
    link = genome[800:870] + rand_seq(rng, 12) + genome[2300:2370]    # a thin bridge between two places of the genome
    c["c_lowedge"] = (["-k", "31", "-D", "1", "-M", "100"], sample_reads(rng, genome, 20) + [link[20:132]] * 3)

    rng = random.Random(404)
    h1 = rand_seq(rng, 3000)
    h2 = list(h1)
    h2[600] = COMP[h2[600]]                                          # SNP
    for p in (2600, 2602, 2604, 2606, 2608, 2610, 2612):             # a stretch too different for -E
        h2[p] = COMP[h2[p]]
    h2 = "".join(h2)
    h2 = h2[:1500] + h2[1504:]                                       # a deletion of 4 bases
    c["d_bubbles"] = (["-k", "31", "-M", "100"], sample_reads(rng, h1, 16) + sample_reads(rng, h2, 11))
    c["e_no_passes"] = (["-k", "31", "-D", "1", "-T", "0", "-W", "0", "-B", "0", "-M", "100"], c["b_tips"][1] + c["c_lowedge"][1][-3:])

    rng = random.Random(606)
    reads = []
    for n in [200] * 12 + [230] * 7 + [170] * 4 + [150, 300]:
        reads += tile_reads(rand_seq(rng, n), 3, step=11)
    c["f_ties"] = (["-k", "31", "-M", "100"], reads)

    rng = random.Random(707)
    c["g_circle"] = (["-k", "31", "-M", "100"], sample_reads(rng, rand_seq(rng, 2000), 18, circular=True) + sample_reads(rng, rand_seq(rng, 1600), 16))

    rng = random.Random(808)
    genome = rand_seq(rng, 1100) + "AAAACCCCGGGGTTTT" + rand_seq(rng, 1000) + "A" * 45 + rand_seq(rng, 900)
    c["h_even_k"] = (["-k", "16", "-M", "100"], sample_reads(rng, genome, 20))

    rng = random.Random(909)
    reads = sample_reads(rng, rand_seq(rng, 3000), 18)
    for n in (110, 118, 125, 140):
        reads += tile_reads(rand_seq(rng, n), 4, step=11)
    c["i_small"] = (["-k", "31", "-M", "125"], reads)

    rng = random.Random(1010)
    c["j_depths"] = (["-k", "31", "-M", "100"], [rand_seq(rng, 140)] * 10 + [rand_seq(rng, 150)] * 62 + sample_reads(rng, rand_seq(rng, 3000), 18))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/DBG_contig")
    ap.add_argument("--scratch", default=None)
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="contig_golden_")
    os.makedirs(scratch, exist_ok=True)
    exe = build_reference(a.ref, scratch)
    ref_dbg = os.path.join(ROOT, "oracle", "_ref", "ref_dbg")
    out_root = os.path.join(HERE, "contig_cases")
    os.makedirs(out_root, exist_ok=True)
    for name, (args, reads) in cases().items():
        args = args + ["-r", "150", "-f", "2", "-i", "0.00002"]
        work = os.path.join(scratch, name)
        os.makedirs(work, exist_ok=True)
        fasta = "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)).encode()
        with open(os.path.join(work, "reads.fa"), "wb") as f:
            f.write(fasta)
        lib = os.path.join(work, "reads.lib")
        with open(lib, "w") as f:
            f.write(os.path.join(work, "reads.fa") + "\n")
        for s in SUFFIXES:       # a pass that is switched off writes no file
            if os.path.exists(os.path.join(work, "out.contig." + s)):
                os.remove(os.path.join(work, "out.contig." + s))
        p = subprocess.run([exe] + args + ["-t", "1", "-o", os.path.join(work, "out"), lib], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        err = "\n".join(ln for ln in p.stderr.decode().split("\n") if "Run time:" not in ln).replace(work, "WORK")
        err = err[err.index("Start to calulate kmer links information!"):]     # the contig stage's part
        outputs = {s: open(os.path.join(work, "out.contig." + s), "rb").read() for s in SUFFIXES if os.path.exists(os.path.join(work, "out.contig." + s))}
        # the reference's table, slot for slot
        img = os.path.join(work, "table.img")
        graph_args = [x for pair in zip(args[::2], args[1::2]) if pair[0] in ("-k", "-r", "-f", "-i") for x in pair]
        subprocess.run([ref_dbg, "build"] + graph_args + ["-t", "1", "-T", img, "-q", lib], stdout=subprocess.PIPE, check=True)
        k = int(args[args.index("-k") + 1])
        t = R.Table.from_image(open(img, "rb").read(), k)
        slots = [i for i in range(t.size) if t.filled[i]]
        case = {"k": k, "table_size": np.uint64(t.size), "slots": np.array(slots, dtype=np.uint32), "kmers": np.array([t.kmer[i] for i in slots], dtype=np.uint64),
                "l_links": np.array([t.l_link[i] for i in slots], dtype=np.uint32), "r_links": np.array([t.r_link[i] for i in slots], dtype=np.uint32)}
        # what the case shows
        o = R.Options.from_args(args)
        files, _, contigs = R.run_stage(R.Table.from_case(case), o)
        t2 = R.Table.from_case(case)
        R.run_stage(t2, o)   # t2: the table after simplification, before the read-out (run_stage reads out on a copy of the flags)
        host_nodes = R.order_dependent_nodes(t2)
        shows = {
            "restatement_equal": all(outputs.get(s) == files.get(s) for s in SUFFIXES),
            "contigs": len(contigs),
            "host_walked_contigs": sum(1 for cc in contigs if cc["anchor"] in host_nodes),
            "branch_unique": b"branch-Unique" in files["seq.fa"], "branch_repeat": b"branch-Repeat" in files["seq.fa"],
            "tips": files.get("tip.fa", b"").count(b">"), "lowedges": files.get("lowedge.fa", b"").count(b">"),
            "bubbles_snp": files.get("bubble.fa", b"").count(b"type: SNP"), "bubbles_indel": files.get("bubble.fa", b"").count(b"type: INDEL"),
            "tips_cut_at_I": files.get("tip.fa", b"").count(b"\tlength: %d\t" % (o.I + k)),
            "small": files["small.fa"].count(b">"),
            "equal_lengths": len(contigs) - len(set(len(cc["bases"]) for cc in contigs)),
            "depth_9": any(9 in cc["depths"] for cc in contigs), "depth_61": any(61 in cc["depths"] for cc in contigs),
            "key0_links": any(t.filled[i] and t.kmer[i] == 0 and (t.l_link[i] or t.r_link[i]) for i in range(t.size)),
            "palindrome": k % 2 == 0 and any(t.filled[i] and t.kmer[i] == R.revcomp(t.kmer[i], k) and t.kmer[i] for i in range(t.size)),
            "kept": t2.kept,
            "break_end_kmers_zero": all(t2.kmer_at(cc[e]) == 0 for cc in contigs for e in ("left_end", "right_end") if cc[e] == t2.size),
        }
        as_bytes = lambda b: np.frombuffer(b, dtype=np.uint8)   # noqa: E731
        arrays = {f: case[f] for f in ("table_size", "slots", "kmers", "l_links", "r_links")}
        arrays.update(args=as_bytes(json.dumps(args).encode()), shows=as_bytes(json.dumps(shows, sort_keys=True).encode()), stderr=as_bytes(err.encode("latin-1")),
                      reads=as_bytes(fasta))
        arrays.update({"out." + s: as_bytes(b) for s, b in outputs.items()})
        np.savez_compressed(os.path.join(out_root, name + ".npz"), **arrays)
        print(name, json.dumps(shows, sort_keys=True))
        assert shows["restatement_equal"], name
        check(name, shows)


def check(name, s):
    """every case shows what it pins"""
    want = {
        "a_repeat": s["branch_unique"] and s["branch_repeat"],
        "b_tips": s["tips"] > 0 and s["kept"]["deep_tips"] > 0 and s["tips_cut_at_I"] > 0,
        "c_lowedge": s["lowedges"] > 0,
        "d_bubbles": s["bubbles_snp"] > 0 and s["bubbles_indel"] > 0 and s["kept"]["diverged_bubbles"] > 0,
        "e_no_passes": s["tips"] == 0 and s["lowedges"] == 0 and s["bubbles_snp"] + s["bubbles_indel"] == 0,
        "f_ties": s["equal_lengths"] >= 17 and s["contigs"] > 16,
        "g_circle": s["host_walked_contigs"] > 0,
        "h_even_k": s["key0_links"] and s["palindrome"],
        "i_small": s["small"] > 0 and s["contigs"] > s["small"],
        "j_depths": s["depth_9"] and s["depth_61"],
    }[name]
    assert want, (name, s)
    if name[0] in "abcdefij":
        assert s["host_walked_contigs"] == 0, (name, s)   # the reference's walk over these inputs meets no order-dependent structure


if __name__ == "__main__":
    main()
