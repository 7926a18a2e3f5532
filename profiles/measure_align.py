#!/usr/bin/env python3
"""Measures the bubbles pass of the contig stage with its alignments computed on the GPU against the same binary with the test hook
align_host=1 (nothing submitted: every alignment on the host, one after another) and, where one is given, against the parent commit's
binary, on one synthetic diploid genome made here: a random haplotype and a copy of it with a deletion of 1..8 bases every `--spacing`
bases, 16x and 11x of 150-bp reads without errors, so that every deletion is an indel bubble and every bubble needs one alignment.
The size is fixed here (--genome 4000000 --spacing 150: about 26 000 bubbles) and recorded; see "job" in the output for what the
bubbles pass took with align_host=1 -- the host's alignments of arms this short are a small part of it.

Three runs of each, through DBGK_TIMINGS: the wall time of the bubbles pass (`Contig stage host passes`: tracing, collecting, aligning,
the ordered loop and the update of the device copy), the counts, device ms and bytes of `Contig stage aligned arms`.  The spread of the
three runs is the margin: "device_faster_than_align_host" is true only when the slowest device run beats the fastest align_host run.
A second part times the kernel alone through capi.ContigBuilder.align on pairs like the stage's (arms of 32..40 letters) and on pairs at
the bound: device ms, pairs/s and cell updates/s from dbgk_align_timing.  Figures that could not be taken are listed under "missing".

    python profiles/measure_align.py [--genome N] [--spacing N] [--parent-bin PATH] [--out profiles/align_measure.json]
"""
import argparse
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin", "debruijn_contig")
ARGS = ["-k", "31", "-r", "150", "-f", "2", "-t", "8", "-i", "0.05", "-M", "125"]     # -D 2, -U 100, -L 0.1, -E 0.1: the defaults
COMP = str.maketrans("ACGT", "TGCA")
RUNS = 3


def write_reads(path, genome_len, spacing, seed=1):
    rng = random.Random(seed)
    h1 = "".join(rng.choices("ACGT", k=genome_len))
    parts, at, n_indels = [], 0, 0
    for p in range(spacing, genome_len - spacing, spacing):
        parts.append(h1[at:p])
        at = p + rng.randrange(1, 9)
        n_indels += 1
    parts.append(h1[at:])
    h2 = "".join(parts)
    with open(path, "w") as f:
        n = 0
        for hap, cov in ((h1, 16), (h2, 11)):
            for _ in range(int(len(hap) * cov / 150)):
                p = rng.randrange(len(hap) - 150)
                r = hap[p:p + 150]
                f.write(">r%d\n%s\n" % (n, r if rng.random() < 0.5 else r.translate(COMP)[::-1]))
                n += 1
    return n_indels, n


def run(exe, lib, prefix, hooks):
    env = dict(os.environ, DBGK_TIMINGS="1")
    if hooks:
        env["DBGK_TEST_HOOKS"] = hooks
    t0 = time.time()
    r = subprocess.run([exe] + ARGS + ["-o", prefix, lib], capture_output=True, text=True, env=env)
    out = {"exit": r.returncode, "program_wall_s": time.time() - t0}
    h = re.search(r"Contig stage host passes \(ms\): first pass (\S+) tips (\S+) low edges (\S+) bubbles (\S+) read-out", r.stderr)
    if h:
        out["bubbles_pass_ms"] = float(h.group(4))
    m = re.search(r"Contig stage aligned arms \(bubbles\): candidates (\d+) submitted (\d+) too long (\d+) used (\d+) aligned on the host (\d+) "
                  r"device ms (\S+) bytes copied back (\d+)", r.stderr)
    if m:
        out["aligned_arms"] = dict(zip(("candidates", "submitted", "too_long", "used", "aligned_on_the_host"), map(int, m.groups()[:5])),
                                   device_ms=float(m.group(6)), bytes_copied_back=int(m.group(7)))
    m = re.search(r"remove total bubble number:\s+(\d+)", r.stderr)
    if m:
        out["bubbles_removed"] = int(m.group(1))
    return out


def kernel_alone(res):
    """pairs like the stage's and pairs at the bound through capi.ContigBuilder.align; three calls each, after one to warm up"""
    from dbg_assembly_amd import capi
    rng = random.Random(7)

    def related(n, m):
        s = "".join(rng.choices("ACGT", k=n))
        p = rng.randrange(1, n - (n - m) - 1) if n > m else 0
        return s, s[:p] + s[p + n - m:]
    sets = {"arms_32_to_40": [related(rng.randrange(33, 41), 32) for _ in range(100000)],
            "at_the_bound_256": [related(capi.ALIGN_MAX_LEN, capi.ALIGN_MAX_LEN - 8) for _ in range(20000)]}
    with capi.ContigBuilder(31) as g:
        for name, pairs in sets.items():
            g.align(pairs[:1000])
            runs = []
            for _ in range(RUNS):
                before = g.align_timing()
                t0 = time.time()
                g.align(pairs)
                wall = time.time() - t0
                now = g.align_timing()
                ms, cells = now["ms_align"] - before["ms_align"], now["cells"] - before["cells"]
                runs.append({"device_ms": ms, "call_wall_ms": wall * 1e3, "pairs_per_s": len(pairs) / (ms * 1e-3), "cell_updates_per_s": cells / (ms * 1e-3),
                             "bytes_up": now["bytes_up"] - before["bytes_up"], "bytes_back": now["bytes_back"] - before["bytes_back"]})
            res["kernel_alone"][name] = {"pairs": len(pairs), "cells": cells, "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4000000)
    ap.add_argument("--spacing", type=int, default=150)
    ap.add_argument("--parent-bin", default=None, help="debruijn_contig of the parent commit, built beside its own lib/")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_measure.json"))
    a = ap.parse_args()
    res = {"job": {"genome": a.genome, "indel_spacing": a.spacing, "indel_lengths": "1..8", "coverage": "16x + 11x", "read_length": 150, "k": 31,
                   "options": " ".join(ARGS), "runs_each": RUNS}, "missing": [], "kernel_alone": {}}
    configs = [("device", BIN, ""), ("align_host", BIN, "align_host=1")]
    if a.parent_bin:
        configs.append(("parent", a.parent_bin, ""))
    else:
        res["missing"].append("parent: no --parent-bin given")
    with tempfile.TemporaryDirectory() as d:
        reads, lib = os.path.join(d, "reads.fa"), os.path.join(d, "reads.lib")
        res["job"]["indels"], res["job"]["reads"] = write_reads(reads, a.genome, a.spacing)
        open(lib, "w").write(reads + "\n")
        for n in range(RUNS):                                   # interleaved, so that a drift of the machine touches all alike
            for name, exe, hooks in configs:
                res.setdefault(name, []).append(run(exe, lib, os.path.join(d, name), hooks))
                sys.stderr.write("%s run %d: %s\n" % (name, n, json.dumps(res[name][-1])))
        done = [name for name, _, _ in configs if all(r["exit"] == 0 and "bubbles_pass_ms" in r for r in res[name])]
        if len(done) == len(configs):
            res["same_files"] = all(open(os.path.join(d, "device.contig." + s), "rb").read() == open(os.path.join(d, name + ".contig." + s), "rb").read()
                                    for name in done[1:] for s in ("bubble.fa", "seq.fa", "seq.depth", "small.fa", "small.depth"))
    for name, _, _ in configs:
        if name in done:
            ms = [r["bubbles_pass_ms"] for r in res[name]]
            res.setdefault("bubbles_pass_ms", {})[name] = {"runs": ms, "min": min(ms), "max": max(ms), "spread": max(ms) - min(ms)}
        else:
            res["missing"].append("bubbles_pass_ms of " + name + ": the program did not run here")
    b = res.get("bubbles_pass_ms", {})
    if "device" in b and "align_host" in b:
        res["job"]["bubbles_pass_ms_with_align_host"] = b["align_host"]["runs"]
        res["device_faster_than_align_host"] = b["device"]["max"] < b["align_host"]["min"]
    if "device" in b and "parent" in b:
        res["device_faster_than_parent"] = b["device"]["max"] < b["parent"]["min"]
    if not b:
        res["note"] = "bin/debruijn_contig did not run here: the figures are not measured"
    try:
        kernel_alone(res)
    except Exception as e:      # no device, or a build without the calls
        res["missing"].append("kernel_alone: %s" % e)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
