#!/usr/bin/env python3
"""Writes tests/golden/simplify_cases/: six inputs in which a removal of a simplification pass reaches into a later walk of the same
pass, each with what the REAL reference program wrote at -t 1 (built as tests/golden/make_contig_golden.py builds it), in the format
of tests/golden/contig_cases (contig_restatement.load_case reads it).

Each case pins one ordering that the validation of traced paths must get right (tests/simplify_restatement.py states the rule), and
check() asserts on the restated passes' event log that the case really shows it:
  a_two_tips_one_node      two tips on one branch node: removing the first makes the node linear, the second walk runs through it
  b_facing_tips            two tips facing each other on an isolated chain: the second starts on the first one's `last`
  c_last_on_earlier_tip    a chain longer than -I: the second tip's `last` (at the cutoff) lies on the first tip's removed path
  d_lowedges_one_end       two low edges that end on one node
  e_bubble_after_bubble    two bubbles with one node between them: the first removal cuts that node's 2 + 2 edges to 1 + 2, which makes
                           it the branch node of the second bubble, whose arms were traced before the cut
  f_tip_and_bubble         two tips and a bubble on one node: the tips pass cuts its 4 edges to the bubble's 2

    python tests/golden/make_simplify_golden.py --ref DIR [--scratch DIR]
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
import contig_restatement as R  # noqa: E402
import simplify_restatement as S  # noqa: E402
from make_contig_golden import COMP, SUFFIXES, build_reference, rand_seq, sample_reads  # noqa: E402

ARGS = ["-k", "31", "-D", "1", "-M", "100"]          # -I -C -U 100, -P -G 3


def other_bases(*taken):
    return [b for b in "ACGT" if b not in taken]


def cases():
    c = {}
    rng = random.Random(1101)
    stem = rand_seq(rng, 60)
    x, y = rng.sample("ACGT", 2)
    c["a_two_tips_one_node"] = sample_reads(rng, rand_seq(rng, 1500), 20) + [stem + x + rand_seq(rng, 30)] * 3 + [stem + y + rand_seq(rng, 30)] * 3

    rng = random.Random(1202)
    c["b_facing_tips"] = sample_reads(rng, rand_seq(rng, 1500), 20) + [rand_seq(rng, 80)] * 3

    rng = random.Random(1303)
    c["c_last_on_earlier_tip"] = sample_reads(rng, rand_seq(rng, 1500), 20) + [rand_seq(rng, 150)] * 3

    rng = random.Random(1404)
    g = rand_seq(rng, 3000)
    # both bridges enter the genome at the k-mer g[2300:2331], each by a base of its own that is not the genome's
    e1, e2 = other_bases(g[2299])[:2]
    bridges = [g[820:870] + other_bases(g[870])[0] + rand_seq(rng, 10) + e1 + g[2300:2350],
               g[1520:1570] + other_bases(g[1570])[0] + rand_seq(rng, 10) + e2 + g[2300:2350]]
    c["d_lowedges_one_end"] = sample_reads(rng, g, 20) + [b for b in bridges for _ in range(3)]

    rng = random.Random(1505)
    h1 = rand_seq(rng, 3000)
    h2 = list(h1)
    for p in (1000, 1032):                            # k + 1 apart: exactly one k-mer lies between the two bubbles
        h2[p] = COMP[h2[p]]
    c["e_bubble_after_bubble"] = sample_reads(rng, h1, 16) + sample_reads(rng, "".join(h2), 11)

    rng = random.Random(1606)
    h1 = rand_seq(rng, 3000)
    h2 = h1[:1000] + COMP[h1[1000]] + h1[1001:]
    x, y = other_bases(h1[1000], h2[1000])
    c["f_tip_and_bubble"] = (sample_reads(rng, h1, 16) + sample_reads(rng, h2, 11)
                             + [h1[940:1000] + x + rand_seq(rng, 30)] * 3 + [h1[940:1000] + y + rand_seq(rng, 30)] * 3)
    return c


def fall_backs(ps):
    """-> [(walk event, removals before it, removals after it)] of the walks that fell back"""
    out = []
    for n, (kind, ev) in enumerate(ps.log):
        if kind == "walk" and not ev["used"]:
            out.append((ev, [e for k2, e in ps.log[:n] if k2 == "removal"], [e for k2, e in ps.log[n:] if k2 == "removal"]))
    return out


def check(name, passes, size):
    """every case shows the ordering it pins"""
    tips, low, bub = (fall_backs(passes[p]) for p in ("tips", "low edges", "bubbles"))
    recalculated = lambda before: {v for e in before for v in e["recalculated"]}   # noqa: E731
    deleted = lambda before: {v for e in before for v in e["nodes"]}               # noqa: E731
    traced = lambda ev: ev["traced"] is not None                                   # noqa: E731
    if name == "a_two_tips_one_node":        # the traced walk ended on the branch node; the live one runs through it
        ok = any(traced(ev) and ev["last_changed"] and not ev["nodes_changed"] and ev["traced"][4] in recalculated(before)
                 and ev["live"][0] > ev["traced"][0] and ev["traced"][4] in ev["live"][2] for ev, before, _ in tips)
    elif name == "b_facing_tips":            # the second tip starts where the first one ended, on a dead end
        ok = any(before and ev["start"] == before[-1]["recalculated"][0] and before[-1]["nodes"][0] != ev["start"]
                 and (not traced(ev) or ev["traced"][4] == before[-1]["nodes"][0]) for ev, before, _ in tips)
    elif name == "c_last_on_earlier_tip":    # both walks stop at the cutoff; the second one's last is a node the first removal deleted
        ok = any(traced(ev) and ev["traced"][0] == 100 and ev["last_changed"] and ev["traced"][4] in deleted(before) for ev, before, _ in tips)
    elif name == "d_lowedges_one_end":       # a later low edge whose end (or branching node) an earlier low edge's removal recalculated, removed too
        ok = any(before and after and (set(after[0]["recalculated"]) & set(before[-1]["recalculated"]))
                 and (ev["branch_changed"] or (traced(ev) and ev["last_changed"])) and not (traced(ev) and ev["nodes_changed"])
                 for ev, before, after in low) and sum(1 for k2, _ in passes["low edges"].log if k2 == "removal") >= 2
    elif name == "e_bubble_after_bubble":    # the node between the bubbles: recalculated by the first removal, the branch of the second
        ok = any(before and after and ev["branch_changed"] and ev["branch"] in before[-1]["recalculated"] and after[0]["recalculated"][1] == ev["branch"]
                 for ev, before, after in bub)
    elif name == "f_tip_and_bubble":         # the node of the two tips is the bubble's branch node or its end
        hit = {ev["traced"][4] for ev, before, _ in tips if traced(ev) and ev["last_changed"] and ev["traced"][4] in recalculated(before)}
        ok = any(set(e["recalculated"]) & hit for k2, e in passes["bubbles"].log if k2 == "removal")
    assert ok, name
    assert sum(len(x) for x in (tips, low, bub)) > 0, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's DBG_contig source directory")
    ap.add_argument("--scratch", default=None)
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="simplify_golden_")
    os.makedirs(scratch, exist_ok=True)
    exe = build_reference(a.ref, scratch)
    ref_dbg = os.path.join(ROOT, "oracle", "_ref", "ref_dbg")
    out_root = os.path.join(HERE, "simplify_cases")
    os.makedirs(out_root, exist_ok=True)
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
        passes = {}
        traced_files, counts, _ = S.run_passes(R.Table.from_case(case), o, passes=passes)
        shows = {
            "restatement_equal": all(outputs[s] == files.get(s) for s in SUFFIXES) and all(outputs[s] == b for s, b in traced_files.items()),
            "tips": files["tip.fa"].count(b">"), "lowedges": files["lowedge.fa"].count(b">"),
            "bubbles_snp": files["bubble.fa"].count(b"type: SNP"), "bubbles_indel": files["bubble.fa"].count(b"type: INDEL"),
            "counts": {p: list(v) for p, v in counts.items()},
        }
        as_bytes = lambda b: np.frombuffer(b, dtype=np.uint8)   # noqa: E731
        arrays = {f: case[f] for f in ("table_size", "slots", "kmers", "l_links", "r_links")}
        arrays.update(args=as_bytes(json.dumps(args).encode()), shows=as_bytes(json.dumps(shows, sort_keys=True).encode()), stderr=as_bytes(err.encode("latin-1")),
                      reads=as_bytes(fasta))
        arrays.update({"out." + s: as_bytes(b) for s, b in outputs.items()})
        np.savez_compressed(os.path.join(out_root, name + ".npz"), **arrays)
        print(name, json.dumps(shows, sort_keys=True))
        assert shows["restatement_equal"], name
        check(name, passes, t.size)


if __name__ == "__main__":
    main()
