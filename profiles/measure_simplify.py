#!/usr/bin/env python3
"""Measures the three simplification passes of the contig stage with their paths traced on the GPU against the same binary with the
test hook simplify_host=1 (every path walked on the host: the code path before tracing), on one synthetic genome made here (3 Mb,
30x, 150-bp reads with substitution errors; -D 0, so that every error k-mer is a node and every error makes a tip or a bubble:
thousands of each).  Writes profiles/simplify_measure.json: per pass the host ms of both runs (the DBGK_TIMINGS line `Contig stage
host passes`), the device ms, requests, traces used and fallen back (`Contig stage traced paths`), the removals the stage counted,
and the whole stage's wall time.  Figures that could not be taken are listed under "missing".

    python profiles/measure_simplify.py [--genome 3000000] [--coverage 30] [--error 0.0002] [--out profiles/simplify_measure.json]
"""
import argparse
import json
import os
import random
import re
import subprocess
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin", "debruijn_contig")
ARGS = ["-k", "31", "-r", "150", "-f", "2", "-t", "8", "-i", "0.05", "-D", "0", "-M", "125"]
PASSES = ("tips", "low edges", "bubbles")


def write_reads(path, genome_len, coverage, error, seed=1):
    rng = random.Random(seed)
    genome = "".join(rng.choices("ACGT", k=genome_len))
    comp = str.maketrans("ACGT", "TGCA")
    with open(path, "w") as f:
        for i in range(int(genome_len * coverage / 150)):
            p = rng.randrange(genome_len - 150)
            r = genome[p:p + 150]
            n_err = sum(1 for _ in range(3) if rng.random() < error * 50)     # at most 3 errors per read, error * 150 on average
            if n_err:
                r = list(r)
                for _ in range(n_err):
                    q = rng.randrange(150)
                    r[q] = rng.choice([b for b in "ACGT" if b != r[q]])
                r = "".join(r)
            f.write(">r%d\n%s\n" % (i, r if rng.random() < 0.5 else r.translate(comp)[::-1]))


def run(lib, prefix, hooks):
    env = dict(os.environ, DBGK_TIMINGS="1")
    if hooks:
        env["DBGK_TEST_HOOKS"] = hooks
    cmd = [BIN] + ARGS + ["-o", prefix, lib]
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    wall = time.time() - t0
    err = r.stderr
    out = {"exit": r.returncode, "program_wall_s": wall, "command": ("DBGK_TIMINGS=1 " + ("DBGK_TEST_HOOKS=%s " % hooks if hooks else "") + " ".join(cmd[:len(ARGS) + 1]) + " -o <prefix> <reads.lib>")}
    h = re.search(r"Contig stage host passes \(ms\): first pass (\S+) tips (\S+) low edges (\S+) bubbles (\S+) read-out (\S+) headers, sort and files (\S+)", err)
    if h:
        v = list(map(float, h.groups()))
        out["host_ms"] = dict(zip(("first_pass", "tips", "low edges", "bubbles", "read_out", "headers_sort_files"), v))
        out["stage_ms"] = sum(v)
    out["traced"] = {m.group(1): {"requests": int(m.group(2)), "used": int(m.group(3)), "fell_back": int(m.group(4)), "device_ms": float(m.group(5)),
                                  "bytes_back": int(m.group(6))}
                     for m in re.finditer(r"Contig stage traced paths \((tips|low edges|bubbles)\): requests (\d+) traces used (\d+) fell back to the host walk (\d+) "
                                          r"device ms (\S+) bytes copied back (\d+)", err)}
    out["removed"] = {name: int(m.group(1)) for name in ("tip", "lowCovEdge", "bubble") for m in [re.search(r"remove total %s number:\s+(\d+)" % name, err)] if m}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=3000000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--error", type=float, default=0.0002)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_measure.json"))
    a = ap.parse_args()
    res = {"job": {"genome": a.genome, "coverage": a.coverage, "read_length": 150, "error_per_base": a.error, "k": 31, "options": " ".join(ARGS)}, "missing": []}
    with tempfile.TemporaryDirectory() as d:
        reads, lib = os.path.join(d, "reads.fa"), os.path.join(d, "reads.lib")
        write_reads(reads, a.genome, a.coverage, a.error)
        open(lib, "w").write(reads + "\n")
        res["host_walk"] = run(lib, os.path.join(d, "host"), "simplify_host=1")
        res["traced"] = run(lib, os.path.join(d, "traced"), "")
        same = all(open(os.path.join(d, "host.contig." + s), "rb").read() == open(os.path.join(d, "traced.contig." + s), "rb").read()
                   for s in ("tip.fa", "lowedge.fa", "bubble.fa", "seq.fa", "seq.depth", "small.fa", "small.depth")) if res["host_walk"]["exit"] == res["traced"]["exit"] == 0 else None
        res["same_files"] = same
    ok = "host_ms" in res["host_walk"] and "host_ms" in res["traced"] and len(res["traced"]["traced"]) == 3
    if ok:
        res["per_pass"] = {p: {"host_ms_with_simplify_host": res["host_walk"]["host_ms"][p], "host_ms_with_tracing": res["traced"]["host_ms"][p],
                               "device_ms": res["traced"]["traced"][p]["device_ms"],
                               "share_fell_back": res["traced"]["traced"][p]["fell_back"] / max(1, res["traced"]["traced"][p]["fell_back"] + res["traced"]["traced"][p]["used"])}
                           for p in PASSES}
        res["stage_wall_ms"] = {"simplify_host": res["host_walk"]["stage_ms"], "traced": res["traced"]["stage_ms"]}
        res["traced_passes_faster"] = all(v["host_ms_with_tracing"] < v["host_ms_with_simplify_host"] for v in res["per_pass"].values())
    else:
        res["missing"] += ["per_pass", "stage_wall_ms", "traced_passes_faster"]
        res["note"] = "bin/debruijn_contig did not run here: the figures are not measured"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
