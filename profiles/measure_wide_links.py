#!/usr/bin/env python3
"""Measures the first pass of the contig stage for k = 63 done on the device with the table (the default) against the same binary with
DBGK_LINKS=0 (the stage's single-threaded pass over the host table), on a table of the cfg5-share size bench.py uses (1.6 G slots
of 32 bytes).  Both passes visit every slot, so their time is set by the table size and not by how many nodes it holds: the input is a
small synthetic genome made here (--genome, 20x of 150-bp reads without errors), which keeps the graph stage short.

Three runs of each through DBGK_TIMINGS: the `first pass` figure of `Contig stage host passes (ms)` (with the device pass: adopting
the lists and writing the frequency file; with DBGK_LINKS=0: the host loop as well), the `host table` figure of `Host phases (s)` (the
export, which with the device pass also holds the two link launches, the copy of the records and the patch of the placed nodes), and
the device time of the two launches (`dbgk wide link pass, device (ms)`).  The spread of the three runs is the margin:
"device_pass_faster" is true only when the slowest default run beats the fastest DBGK_LINKS=0 run on first pass + host table.
Figures that could not be taken are listed under "missing".  The result file is rewritten after every run; every run has a time limit
(--run-timeout), and after a run that fails or is killed nothing more is started.

    python profiles/measure_wide_links.py [--slots-g 1.6] [--genome 2000000] [--run-timeout 300] [--note TEXT] [--out profiles/wide_links_measure.json]
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
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin", "debruijn_contig")
COMP = str.maketrans("ACGT", "TGCA")
RUNS = 3


def write_reads(path, genome_len, seed=1):
    rng = random.Random(seed)
    g = "".join(rng.choices("ACGT", k=genome_len))
    n = genome_len * 20 // 150
    with open(path, "w") as f:
        for i in range(n):
            p = rng.randrange(len(g) - 150)
            r = g[p:p + 150]
            f.write(">r%d\n%s\n" % (i, r if rng.random() < 0.5 else r.translate(COMP)[::-1]))
    return n


def run(args, lib, prefix, links, timeout):
    env = dict(os.environ, DBGK_TIMINGS="1")
    env.pop("DBGK_LINKS", None)
    if links is not None:
        env["DBGK_LINKS"] = links
    t0 = time.time()
    try:
        r = subprocess.run([BIN] + args + ["-o", prefix, lib], capture_output=True, text=True, env=env, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {"exit": None, "killed_after_s": timeout}
    out = {"exit": r.returncode, "program_wall_s": round(time.time() - t0, 3), "pass_on_the_gpu": "First pass of the contig stage done on the GPU" in r.stderr}
    m = re.search(r"Contig stage host passes \(ms\): first pass (\S+)", r.stderr)
    if m:
        out["first_pass_ms"] = float(m.group(1))
    m = re.search(r"Host phases \(s\):.* host table (\S+)", r.stderr)
    if m:
        out["host_table_s"] = float(m.group(1))
    m = re.search(r"dbgk wide link pass, device \(ms\): records, flags and counts (\S+), lists (\S+) \(", r.stderr)
    if m:
        out["link_launches_device_ms"] = {"records_flags_counts": float(m.group(1)), "lists": float(m.group(2))}
    m = re.search(r"^array_size: (\d+)", r.stderr, re.M)
    if m:
        out["table_slots"] = int(m.group(1))
    if r.returncode != 0:
        out["stderr_tail"] = r.stderr[-400:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots-g", type=float, default=1.6, help="-i of the program: table slots in units of 1e9 (bench.py's cfg5 share: 1.6)")
    ap.add_argument("--genome", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_links_measure.json"))
    ap.add_argument("--run-timeout", type=float, default=300, help="seconds after which one run of the program is ended")
    ap.add_argument("--note", default="", help="free text kept in the result file (the machine, why a figure is missing, ...)")
    a = ap.parse_args()
    args = ["-k", "63", "-r", "150", "-f", "2", "-t", "8", "-i", repr(a.slots_g), "-M", "125"]
    res = {"job": {"k": 63, "table_slots_asked_g": a.slots_g, "genome": a.genome, "coverage": "20x", "read_length": 150, "options": " ".join(args),
                   "runs_each": RUNS}, "note": a.note, "missing": [], "device_pass": [], "links_0_host_pass": []}

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    with tempfile.TemporaryDirectory() as d:
        fa, lib = os.path.join(d, "reads.fa"), os.path.join(d, "reads.lib")
        res["job"]["reads"] = write_reads(fa, a.genome)
        with open(lib, "w") as f:
            f.write(fa + "\n")
        # alternating, so that a drift of the machine touches both alike; nothing more is started after a run that failed or was killed
        for i, (name, links) in enumerate([("device_pass", None), ("links_0_host_pass", "0")] * RUNS):
            res[name].append(run(args, lib, os.path.join(d, "out_%d" % i), links, a.run_timeout))
            print(name, i // 2, res[name][-1], flush=True)
            save()
            if res[name][-1]["exit"] != 0:
                res["stopped"] = "after run %d of %s: exit %s" % (i // 2, name, res[name][-1]["exit"])
                break
    for name in ("device_pass", "links_0_host_pass"):
        for field in ("first_pass_ms", "host_table_s"):
            if len(res[name]) < RUNS or not all(field in r and r["exit"] == 0 for r in res[name]):
                res["missing"].append("%s of %s: not every run gave it" % (field, name))
    if len(res["device_pass"]) < RUNS or not all("link_launches_device_ms" in r for r in res["device_pass"]):
        res["missing"].append("link_launches_device_ms: not every run gave it")
    if not res["missing"]:
        total = lambda r: r["first_pass_ms"] + 1e3 * r["host_table_s"]   # noqa: E731
        dev, host = [total(r) for r in res["device_pass"]], [total(r) for r in res["links_0_host_pass"]]
        res["first_pass_plus_host_table_ms"] = {"device_pass": dev, "links_0_host_pass": host}
        res["device_pass_faster"] = max(dev) < min(host)
    save()
    print(json.dumps(res.get("first_pass_plus_host_table_ms", res["missing"])))


if __name__ == "__main__":
    sys.exit(main())
