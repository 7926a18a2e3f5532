"""bin/map_reads and bin/map_pair file to file with DBGK_TEXT=device, and the ROWS stage on its own, on the mapper bullet's workload:
250-base reads with 1 % substitutions on 5 Mb of contigs (profiles/measure_map.py), k = 31, s = 5.

  1. rows in process   the FASTA text of the reads in batches of 1 M: Parser.chunk, Mapper.map_device(keep=True), then the two calls
                       that are new -- RowWriter.take_hits and RowWriter.rows_device -- timed as wall time and as the device time the
                       library reports (token spans + lengths + scans; segments + write kernels).  For the write pass: output bytes
                       read + written per second (twice the stream bytes: every output byte is read once from its source) next to
                       dbgk_measure_copy_bandwidth of the same run.
  2. programs          bin/map_reads on --program-reads reads and bin/map_pair on half as many pairs, each with DBGK_TEXT unset (the
                       host readers and the host loop of flush(), unchanged by this commit) and =device, DBGK_GZ=device in both, plain
                       FASTA files on memory-backed storage.

NOT measured: the host loop of flush() on its own.  It is C++ inside the programs; its cost is part of the programs' figures with the
switch unset, together with the host reader's.

Each run is repeated --reps times, interleaved; the project's rule decides: the slowest run of the new route against the fastest of
the old.  Writes profiles/maprow_measure.json; without a GPU it lists the figures that are missing.  Reported, not gated.

    python profiles/measure_maprow.py [--reads 10000000] [--program-reads 10000000] [--reps 3]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "maprow_measure.json")
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
FIGURES = ["rows in process: wall_s of take_hits + rows_device, device ms_scan / ms_write, stream bytes (3 runs)",
           "write pass GB/s (bytes read + written) and copy_bandwidth GB/s of the same run",
           "bin/map_reads: DBGK_TEXT unset / device wall_s (3 runs each)", "bin/map_pair: DBGK_TEXT unset / device wall_s (3 runs each)",
           "routes_separate"]
GENOME, READ_LEN, BATCH = 5000000, 250, 1000000


def workload(seed=1):
    """the contigs and a batch maker of profiles/measure_map.py"""
    rng = np.random.default_rng(seed)
    whole = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, GENOME)].tobytes()
    contigs = [whole[i:i + 50000] for i in range(0, len(whole), 50000)]
    src = np.frombuffer(whole, dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y

    def make_batch(n, first):
        """n FASTA records ">rNNNNNNNNN 1" / 250 bases as one uint8 array"""
        start = rng.integers(0, len(src) - READ_LEN, n)
        reads = src[start[:, None] + np.arange(READ_LEN)[None, :]].copy()
        err = rng.random(reads.shape) < 0.01
        reads[err] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(err.sum()))]
        reads[1::2] = comp[reads[1::2, ::-1]]
        text = np.empty((n, 14 + READ_LEN + 1), dtype=np.uint8)
        text[:, 0], text[:, 1] = ord(">"), ord("r")
        idx = np.arange(first, first + n, dtype=np.int64)
        for d in range(9):
            text[:, 2 + d] = ord("0") + (idx // 10 ** (8 - d)) % 10
        text[:, 11], text[:, 12], text[:, 13] = ord(" "), ord("1"), 10
        text[:, 14:14 + READ_LEN] = reads
        text[:, 14 + READ_LEN] = 10
        return text.reshape(-1)
    return contigs, make_batch


def rows_in_process(capi, contigs, batches, n_batches, mode):
    pair = mode == capi.MAPROW_PAIR
    names = [b"contig_%d" % i for i in range(len(contigs))]
    res = {"wall_s": 0.0, "ms_scan": 0.0, "ms_write": 0.0, "stream_bytes": [0, 0, 0], "items": 0, "ms_map": 0.0}
    with capi.Mapper(k=31, s=5, r=250, identity=0.97, second_alignment=not pair) as m, capi.RowWriter(mode, b"> \t" if pair else b">@ \t\n", 250) as w:
        m.set_contigs(contigs)
        w.set_contigs(names, [len(c) for c in contigs])
        parsers = [capi.Parser(2) for _ in range(2 if pair else 1)]
        try:
            for b in range(-1, n_batches):   # (-1: a warm-up round that sizes every buffer)
                n = None
                for s, p in enumerate(parsers):
                    info = p.chunk(batches[(b + s) % len(batches)])
                    n = info["n_records"]
                    d_b, _, d_o, _, nb = p.device()
                    m.map_device(d_b, d_o, n, nb, info["max_len"], keep=True)
                    if b >= 0:
                        st = m.batch_stats()
                        res["ms_map"] += st["ms_map"] + st["ms_long"]
                    t0 = time.perf_counter()
                    w.take_hits(s, m)
                    if b >= 0:
                        res["wall_s"] += time.perf_counter() - t0
                t0 = time.perf_counter()
                info = w.rows_device(parsers, n)
                if b >= 0:
                    res["wall_s"] += time.perf_counter() - t0
                    res["ms_scan"] += info["ms_scan"]
                    res["ms_write"] += info["ms_write"]
                    res["items"] += n
                    res["stream_bytes"] = [x + y for x, y in zip(res["stream_bytes"], info["stream_bytes"])]
                    assert info["unprintable"] == 0
        finally:
            for p in parsers:
                p.close()
    out = sum(res["stream_bytes"])
    res["write_gbps_read_plus_written"] = 2 * out / (res["ms_write"] / 1e3) / 1e9 if res["ms_write"] else None
    res["items_per_s_wall"] = res["items"] / res["wall_s"] if res["wall_s"] else None
    return res


def run_program(prog, args, env, cwd):
    """in `cwd`: the library file names its reads files relative to it"""
    t0 = time.perf_counter()
    r = subprocess.run([os.path.join(BIN, prog)] + args, capture_output=True, text=True, env=env, cwd=cwd)
    wall = time.perf_counter() - t0
    assert r.returncode == 0 and "fail to open" not in r.stderr, r.stderr[-2000:]
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--program-reads", type=int, default=10000000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    if capi.lib().dbgk_device_count() < 1:
        json.dump({"missing": FIGURES, "reason": "no GPU"}, open(OUT, "w"), indent=1)
        print("no GPU: wrote the list of missing figures")
        return
    contigs, make_batch = workload()
    batches = [make_batch(BATCH, k * BATCH) for k in range(2)]   # two distinct batches, alternated, as measure_map.py does
    n_batches = max(1, a.reads // BATCH)
    res = {"reads": n_batches * BATCH, "read_len": READ_LEN, "contig_bases": GENOME, "k": 31, "s": 5, "batch": BATCH, "runs": {}}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        res["copy_bandwidth_gbps"] = g.copy_bandwidth(2 << 30, 5)
    for name, mode, nb in (("rows_reads_in_process", capi.MAPROW_READS, n_batches), ("rows_pair_in_process", capi.MAPROW_PAIR, max(1, n_batches // 2))):
        res["runs"][name] = []
        for _ in range(a.reps):
            run = rows_in_process(capi, contigs, batches, nb, mode)
            print(name, json.dumps(run), flush=True)
            res["runs"][name].append(run)
    # the programs: plain FASTA files on memory-backed storage
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=shm) as d:
        open(os.path.join(d, "contigs.fa"), "wb").write(b"".join(b">contig_%d\n%s\n" % (i, c) for i, c in enumerate(contigs)))
        nb = max(1, a.program_reads // BATCH)
        for f, shift in (("reads_1.fa", 0), ("reads_2.fa", 1)):
            with open(os.path.join(d, f), "wb") as out:
                for b in range(nb if f == "reads_1.fa" else max(1, nb // 2)):
                    out.write(batches[(b + shift) % 2].tobytes())
        # (map_pair takes the first half of reads_1.fa's records: its second file is half as long, so its own copy of the first)
        with open(os.path.join(d, "mate_1.fa"), "wb") as out:
            for b in range(max(1, nb // 2)):
                out.write(batches[b % 2].tobytes())
        open(os.path.join(d, "se.lib"), "w").write("reads_1.fa\n")
        open(os.path.join(d, "pe.lib"), "w").write("mate_1.fa\nreads_2.fa\n")
        base = {k: v for k, v in os.environ.items() if k not in ("DBGK_TEXT", "DBGK_GZ", "DBGK_TEST_HOOKS", "DBGK_TIMINGS")}
        res["program_reads"] = nb * BATCH
        for prog, lib in (("map_reads", "se.lib"), ("map_pair", "pe.lib")):
            key_old, key_new = "bin/%s, DBGK_TEXT unset" % prog, "bin/%s, DBGK_TEXT=device" % prog
            res["runs"][key_old], res["runs"][key_new] = [], []
            for rep in range(a.reps):
                for key, env in ((key_old, {}), (key_new, {"DBGK_TEXT": "device"})):
                    out_dir = os.path.join(d, "out_%s_%d_%d" % (prog, rep, len(env)))
                    wall = run_program(prog, ["-f", "2", "-o", out_dir, os.path.join(d, "contigs.fa"), os.path.join(d, lib)],
                                       dict(base, DBGK_GZ="device", **env), d)
                    print(key, wall, flush=True)
                    res["runs"][key].append({"wall_s": wall})
                    subprocess.run(["rm", "-rf", out_dir])
            old, new = [r["wall_s"] for r in res["runs"][key_old]], [r["wall_s"] for r in res["runs"][key_new]]
            res["%s_slowest_new_over_fastest_old" % prog] = max(new) / min(old)
            res["%s_routes_separate" % prog] = max(new) < min(old) or min(new) > max(old)
    res["not_measured"] = ["the host loop of flush() on its own (it is part of the programs' figures with the switch unset)"]
    json.dump(res, open(OUT, "w"), indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
