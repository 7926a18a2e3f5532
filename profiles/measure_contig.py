#!/usr/bin/env python3
"""Measures the contig stage on one synthetic genome of E. coli size (4.6 Mb, 40x, 150-bp reads, k = 31) and writes
profiles/contig_measure.json: device time per read-out kernel and host time per pass (the DBGK_TIMINGS lines of
bin/debruijn_contig), the cost of copying the table to the device again, and -- where oracle/_ref/ref_consumer is built -- the
reference's read-out phase on the same table: the difference of its `Run time:` lines (CPU seconds of clock(), taken at -t 1) around
"Start to read out contig sequence".
Figures that could not be taken are listed under "missing".

    python profiles/measure_contig.py [--genome 4600000] [--coverage 40] [--out profiles/contig_measure.json]
"""
import argparse
import json
import os
import random
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin", "debruijn_contig")
REF = os.path.join(ROOT, "oracle", "_ref", "ref_consumer")
ARGS = ["-k", "31", "-r", "150", "-f", "2", "-t", "8", "-i", "0.05", "-M", "125"]


def write_reads(path, genome_len, coverage, seed=1):
    rng = random.Random(seed)
    genome = "".join(rng.choices("ACGT", k=genome_len))
    comp = str.maketrans("ACGT", "TGCA")
    with open(path, "w") as f:
        for i in range(int(genome_len * coverage / 150)):
            p = rng.randrange(genome_len - 150)
            r = genome[p:p + 150]
            f.write(">r%d\n%s\n" % (i, r if rng.random() < 0.5 else r.translate(comp)[::-1]))


def run(exe, lib, prefix, env, args=ARGS):
    r = subprocess.run([exe] + args + ["-o", prefix, lib], capture_output=True, text=True, env=dict(os.environ, **env))
    return r.returncode, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4600000)
    ap.add_argument("--coverage", type=float, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contig_measure.json"))
    a = ap.parse_args()
    res = {"job": {"genome": a.genome, "coverage": a.coverage, "read_length": 150, "k": 31, "options": " ".join(ARGS)}, "missing": []}
    with tempfile.TemporaryDirectory() as d:
        reads, lib = os.path.join(d, "reads.fa"), os.path.join(d, "reads.lib")
        write_reads(reads, a.genome, a.coverage)
        open(lib, "w").write(reads + "\n")
        rc, err = run(BIN, lib, os.path.join(d, "ours"), {"DBGK_TIMINGS": "1", "DBGK_LAYOUT": "ref"})
        m = re.search(r"Contig read-out \(ms\): upload (\S+) \((\d+) bytes\) compact (\S+) successors (\S+) mutual (\S+) rank (\S+) \((\d+) rounds\) "
                      r"place (\S+) scatter (\S+) emit (\S+) host walk (\S+); contigs by kernels (\d+), by the host walker (\d+)", err)
        h = re.search(r"Contig stage host passes \(ms\): first pass (\S+) tips (\S+) low edges (\S+) bubbles (\S+) read-out (\S+) headers, sort and files (\S+)", err)
        if rc == 0 and m and h:
            g = m.groups()
            res["read_out_ms"] = dict(zip(("compact", "successors", "mutual", "rank", "place", "scatter", "emit", "host_walk"),
                                          map(float, (g[2], g[3], g[4], g[5], g[7], g[8], g[9], g[10]))))
            res["table_upload"] = {"ms": float(g[0]), "bytes": int(g[1]),
                                   "note": "the table is copied to the device again for the read-out; taking the image from the graph handle is not done"}
            res["rounds"], res["kernel_contigs"], res["host_walked_contigs"] = int(g[6]), int(g[11]), int(g[12])
            res["host_ms"] = dict(zip(("first_pass", "tips", "low_edges", "bubbles", "read_out_call", "headers_sort_files"), map(float, h.groups())))
        else:
            res["missing"] += ["read_out_ms", "table_upload", "host_ms"]
            res["note"] = "bin/debruijn_contig did not run here (exit %d): the GPU figures are not measured" % rc
        if os.path.exists(REF) and rc == 0:
            # at -t 1: the reference's `Run time:` lines are clock() CPU seconds, which equal wall time only for one thread
            rc2, err2 = run(REF, lib, os.path.join(d, "ref"), {"DBGK_LAYOUT": "ref"}, [x if x != "8" else "1" for x in ARGS])
            t = [float(x) for x in re.findall(r"Run time: (\S+)", err2[err2.find("Start to calulate"):])]
            if rc2 == 0 and len(t) >= 2:
                res["reference_read_out_cpu_s_at_t1"] = t[-1] - t[-2]   # between the lines around "Start to read out contig sequence"
            else:
                res["missing"].append("reference_read_out_cpu_s_at_t1")
        else:
            res["missing"].append("reference_read_out_cpu_s_at_t1")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
