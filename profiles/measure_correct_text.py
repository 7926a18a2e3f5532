"""bin/correct_error_reads and bin/kmerfreq file to file with DBGK_TEXT=device, against their host readers:

  1. new route, in process   the FASTQ text of N x 150 bp reads (5 Mbp genome, 1 % substitutions) in memory, in windows: upload +
                    Parser.chunk without a quality plane, Corrector.correct_device against a k = 17 table made from a KFREQ handle,
                    compact, annotate_device, Formatter.format_device with the plane where it lies.  Wall time of the whole, the
                    device time of every stage -- the corrector's kernels on their own -- and for the annotation: ms of its two
                    passes per GB of suffixes, and bytes read + written per second next to dbgk_measure_copy_bandwidth of the run.
  2. old route      today's loop of host/correct_error_reads.cpp.  It is NOT restated here: it is the loop this commit's binary runs
                    with DBGK_TEXT unset, unchanged from the parent commit, so the old route is measured as the program, on the same
                    file as (3).  What the program does not print for it is the device time of the corrector's kernels; that figure is
                    the in-process one of (1), the same kernels on the same reads.
  3. programs       bin/correct_error_reads on the N reads and on 1 M of them, bin/kmerfreq on 1 M, each with DBGK_TEXT unset and
                    =device, DBGK_GZ=device in both forms, plain files on memory-backed storage.

Each run is repeated --reps times, interleaved; the project's rule decides: the slowest run of the new route against the fastest of
the old.  Writes profiles/correct_text_measure.json; without a GPU it lists the figures that are missing.  Reported, not gated.

    python profiles/measure_correct_text.py [--reads 10000000] [--program-reads 1000000] [--window 268435456] [--reps 3]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from measure_parse import READ_LEN, rounded  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "correct_text_measure.json")
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
FIGURES = ["new route in process: wall_s and device ms per stage, the corrector's kernels apart (3 runs)",
           "annotation: ms_scan, ms_write per GB of suffixes; write GB/s (bytes read + written); copy_bandwidth GB/s of the same run",
           "bin/correct_error_reads on 10 M reads: DBGK_TEXT unset (the old route) / device wall_s (3 runs each)", "routes_separate",
           "bin/correct_error_reads on 1 M reads: DBGK_TEXT unset / device wall_s (3 runs each)",
           "bin/kmerfreq on 1 M reads: DBGK_TEXT unset / device wall_s (3 runs each)"]
K, CUTOFF, GENOME = 17, 2, 5000000


def make_text(n, capi, g):
    """n records "@rNNNNNNNNN / 150 bases / + / 150 qualities" of reads drawn from one genome, as one uint8 array; the reads are
    pushed into the KFREQ handle g on the way"""
    from oracle import oracle_py as O
    P = O.synth_params(GENOME, READ_LEN, sub_rate=0.01, n_rate=0.002, cfg=11)
    width = 11 + (READ_LEN + 1) + 2 + (READ_LEN + 1)
    text = np.empty((n, width), dtype=np.uint8)
    for a in range(0, n, 1 << 20):
        b = min(n, a + (1 << 20))
        bases, offsets = O.synth_reads(P, a, b - a)
        g.push_reads(bases, offsets)
        t = text[a:b]
        t[:, 0], t[:, 1] = ord("@"), ord("r")
        idx = np.arange(a, b, dtype=np.int64)
        for d in range(9):
            t[:, 2 + d] = ord("0") + (idx // 10 ** (8 - d)) % 10
        t[:, 10] = 10
        t[:, 11:11 + READ_LEN] = bases.reshape(b - a, READ_LEN)
        t[:, 11 + READ_LEN] = 10
        t[:, 12 + READ_LEN], t[:, 13 + READ_LEN] = ord("+"), 10
        t[:, 14 + READ_LEN:14 + 2 * READ_LEN] = ord("I")
        t[:, 14 + 2 * READ_LEN] = 10
    return text.reshape(-1)


def new_route(capi, p, c, f, text, window):
    L = capi.lib()
    ms = {k: 0.0 for k in ("parse", "corrector_kernels", "compact", "annot_scan", "annot_write", "format")}
    reads = out_bytes = suffix_bytes = 0
    t0 = time.perf_counter()
    pos = 0
    while True:
        chunk = text[pos:pos + window]
        last = pos + window >= text.size
        pi = p.chunk(chunk, last)
        n = pi["n_records"]
        offsets = np.empty(n + 1, dtype=np.uint64)
        assert L.dbgk_parse_results(p._h, None, None, offsets.ctypes.data, None) == 0
        d_b = p.device()[0]
        c.correct_device(d_b, offsets)
        st = c.batch_stats()
        ci = c.compact()
        dev = c.annotate_device()
        cb, co, _, _ = c.compact_device()
        fi = f.format_device(p, (cb, None, co, n), dev)
        ms["parse"] += pi["ms_lines"] + pi["ms_states"] + pi["ms_scan"] + pi["ms_gather"]
        ms["corrector_kernels"] += st["ms_classify"] + st["ms_correct"] + st["ms_overflow"]
        ms["compact"] += ci["ms_scan"] + ci["ms_gather"]
        ms["annot_scan"] += c.annot_info["ms_scan"]
        ms["annot_write"] += c.annot_info["ms_write"]
        ms["format"] += fi["ms_scan"] + fi["ms_gather"]
        reads, out_bytes, suffix_bytes = reads + n, out_bytes + fi["out_bytes"], suffix_bytes + dev.n_bytes
        if last:
            break
        assert pi["consumed"] > 0, "the window is smaller than one record"
        pos += pi["consumed"]
    wall = time.perf_counter() - t0
    gb = suffix_bytes / 1e9
    moved = reads * (24 + 8 + 8) + (suffix_bytes + 15) // 16 * 16   # a record, a compact offset and a suffix offset read per suffix written
    return dict(wall_s=wall, reads=reads, out_bytes=out_bytes, suffix_bytes=suffix_bytes, device_ms=ms,
                annot_ms_per_gb={"scan": ms["annot_scan"] / gb, "write": ms["annot_write"] / gb}, annot_write_gbps=moved / (ms["annot_write"] * 1e6))


def program(exe, args, outputs, text_on_device):
    env = {k: v for k, v in os.environ.items() if k not in ("DBGK_TEXT", "DBGK_GUNZIP", "DBGK_TEST_HOOKS", "DBGK_TIMINGS", "DBGK_GPUS", "DBGK_GPU_LIST")}
    env["DBGK_GZ"] = "device"
    if text_on_device:
        env["DBGK_TEXT"] = "device"
    t0 = time.perf_counter()
    subprocess.run([os.path.join(BIN, exe)] + args, check=True, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1200)
    wall = time.perf_counter() - t0
    return {"wall_s": wall, "outputs": {os.path.basename(o): os.path.getsize(o) for o in outputs}}


def verdict_of(new, old):
    slow_new, fast_old = max(r["wall_s"] for r in new), min(r["wall_s"] for r in old)
    return {"slowest_new_s": slow_new, "fastest_old_s": fast_old, "routes_separate": bool(slow_new < fast_old),
            "speedup_slowest_new_vs_fastest_old": fast_old / slow_new}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--program-reads", type=int, default=1000000)
    ap.add_argument("--window", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    job = dict(reads=a.reads, program_reads=a.program_reads, read_len=READ_LEN, k=K, cutoff=CUTOFF, genome=GENOME, window_bytes=a.window, reps=a.reps)
    if capi.lib().dbgk_device_count() < 1:
        with open(a.out, "w") as f:
            json.dump({"job": job, "missing": FIGURES, "note": "no GPU on the machine this file was written on: nothing here is measured"}, f, indent=1)
            f.write("\n")
        print("no GPU: wrote the list of missing figures to", a.out)
        return
    runs = {"new_in_process": [], "correct_host_text": [], "correct_device_text": [], "correct_1m_host_text": [], "correct_1m_device_text": [],
            "kmerfreq_1m_host_text": [], "kmerfreq_1m_device_text": []}
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
        with capi.Graph(k=K, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=1000, expected_kmers=(1 << 20) * 134) as g:
            text = make_text(a.reads, capi, g)
            g.finalize()
            per = text.size // a.reads
            job["text_bytes"] = int(text.size)
            path, small = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "reads_1m.fq")
            text.tofile(path)
            text[:a.program_reads * per].tofile(small)
            print("text written", file=sys.stderr, flush=True)
            with capi.Corrector(k=K) as c, capi.Parser(1, False) as p, capi.Formatter(2, b">") as f:
                c.from_kfreq(g, CUTOFF)
                new_route(capi, p, c, f, text[:min(text.size, 64 << 20) // per * per], a.window)   # first touch of every buffer, not counted
                for _ in range(a.reps):
                    runs["new_in_process"].append(new_route(capi, p, c, f, text, a.window))
                    print("in process:", round(runs["new_in_process"][-1]["wall_s"], 3), file=sys.stderr, flush=True)
                copy_gbps = g.copy_bandwidth(2 << 30, 5)
        del text
        # the table file of the programs: what bin/kmerfreq writes for the whole input
        libs = {}
        for name, reads in (("all", path), ("1m", small)):
            libs[name] = os.path.join(tmp, name + ".lib")
            open(libs[name], "w").write(reads + "\n")
        table = os.path.join(tmp, "all")
        kf = ["-k", str(K), "-f", "1", "-b", "1", "-m", str(CUTOFF)]
        program("kmerfreq", kf + ["-o", table, libs["all"]], [], False)
        table += ".kmer.freq.cz"
        kf_out = [os.path.join(tmp, "kf.kmer.freq" + e) for e in (".cz", ".cz.len", ".stat")]
        program("correct_error_reads", ["-k", str(K), table, libs["1m"]], [], True)   # first run of the binaries, not counted
        for _ in range(a.reps):
            for dev in (False, True):
                tag = "device_text" if dev else "host_text"
                runs["correct_" + tag].append(program("correct_error_reads", ["-k", str(K), table, libs["all"]], [path + ".correct.fa.gz", path + ".correct.stat"], dev))
                runs["correct_1m_" + tag].append(program("correct_error_reads", ["-k", str(K), table, libs["1m"]], [small + ".correct.fa.gz", small + ".correct.stat"], dev))
                runs["kmerfreq_1m_" + tag].append(program("kmerfreq", kf + ["-o", os.path.join(tmp, "kf"), libs["1m"]], kf_out, dev))
            print("programs:", {k: round(v[-1]["wall_s"], 3) for k, v in runs.items() if v and k != "new_in_process"}, file=sys.stderr, flush=True)
    verdict = {"correct_error_reads": verdict_of(runs["correct_device_text"], runs["correct_host_text"]),
               "correct_error_reads_1m": verdict_of(runs["correct_1m_device_text"], runs["correct_1m_host_text"]),
               "kmerfreq_1m": verdict_of(runs["kmerfreq_1m_device_text"], runs["kmerfreq_1m_host_text"])}
    out = {"job": job, "runs": runs, "rule": "the slowest run of the new route against the fastest run of the old", "verdict": verdict,
           "copy_bandwidth_gbps": copy_gbps, "annot_write_over_copy": [r["annot_write_gbps"] / copy_gbps for r in runs["new_in_process"]],
           "bytes_counted": {"annot_write": "per record 24 bytes of record, a compact offset and a suffix offset read, and the 16-byte vectors of suffixes written"},
           "notes": ["the old route is the program with DBGK_TEXT unset: the loop of host/correct_error_reads.cpp, unchanged from the parent commit; it is not restated",
                     "the device time of the corrector's kernels is that of the in-process runs; the host route runs the same kernels on the same reads in batches of 1 M",
                     "the programs run with DBGK_GZ=device in both forms and read plain files from memory-backed storage",
                     "what bounds the annotation's write rate is not profiled"]}
    with open(a.out, "w") as f:
        json.dump(rounded(out), f, indent=1)
        f.write("\n")
    print(json.dumps(rounded({"verdict": verdict, "copy_bandwidth_gbps": copy_gbps, "in_process": runs["new_in_process"]})))


if __name__ == "__main__":
    main()
