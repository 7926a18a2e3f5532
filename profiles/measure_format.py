"""From the device batch to the bytes of the output file on two routes, 10 M x 150 bp FASTQ:

  1. device time    the text of the file in windows: upload, Parser.chunk_device with a quality plane, then Formatter.format_device on
                    the parser's own batch without suffixes, which writes the window's records again.  ms_scan (lengths + scan) and
                    ms_gather summed over the windows, per GB of output, and the gather's bytes read + written per second next to
                    dbgk_measure_copy_bandwidth of the same run.  The wall time of the format calls is the new composition.
  2. old composition  the loop of RecordBatch::write over the same records (profiles/format_old_route.cpp, built here with g++) and
                    the upload of its pieces, which is what DBGK_GZ=device needs today.  Reading the records is not timed.
  3. program        bin/clean_lowqual on 1 M reads of plain FASTQ with DBGK_GZ=device, DBGK_TEXT unset against device.

Each route runs --reps times, interleaved; the project's rule decides: the slowest run of the new route against the fastest of the
old.  Writes profiles/format_measure.json; without a GPU it lists the figures that are missing.  Reported, not gated.

    python profiles/measure_format.py [--reads 10000000] [--program-reads 1000000] [--window 268435456] [--reps 3]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from measure_parse import READ_LEN, make_text, rounded  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "format_measure.json")
FIGURES = ["ms_scan, ms_gather per GB of output (3 runs)", "gather TB/s (bytes read + written)", "copy_bandwidth GB/s of the same run",
           "new composition wall_s (3 runs)", "old composition + upload wall_s (3 runs)", "routes_separate",
           "bin/clean_lowqual 1 M reads, DBGK_GZ=device: DBGK_TEXT unset / device wall_s (3 runs each)", "programs_separate"]
TEXT_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64)


def build_helper(tmp):
    so = os.path.join(tmp, "format_old_route.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "dbg_assembly_amd", "host"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "profiles", "format_old_route.cpp"), "-o", so, "-L" + os.path.join(ROOT, "dbg_assembly_amd", "lib"), "-ldbgk",
                    "-Wl,-rpath," + os.path.join(ROOT, "dbg_assembly_amd", "lib"), "-lz", "-lpthread"], check=True)
    L = ctypes.CDLL(so)
    L.old_compose.restype = ctypes.c_longlong
    L.old_compose.argtypes = [ctypes.c_char_p, TEXT_CB, ctypes.POINTER(ctypes.c_double)]
    return L


def old_route(capi, L, g, path):
    d = g.malloc(256 << 20)
    state = {"upload_s": 0.0, "bytes": 0}

    def take(text, n):
        t0 = time.perf_counter()
        assert n <= d.nbytes
        if n:
            assert capi.lib().dbgk_memcpy_h2d(g._h, d.ptr, ctypes.c_void_p(text), n) == 0
        state["upload_s"] += time.perf_counter() - t0
        state["bytes"] += n
    try:
        s = ctypes.c_double(0)
        n = L.old_compose(path.encode(), TEXT_CB(take), ctypes.byref(s))
        return {"wall_s": s.value, "upload_s": state["upload_s"], "compose_s": s.value - state["upload_s"], "reads": n, "out_bytes": state["bytes"]}
    finally:
        d.free()


def new_route(capi, g, p, f, text, window):
    d = g.malloc(window + 16)
    ms = {"ms_scan": 0.0, "ms_gather": 0.0}
    wall = 0.0
    reads = out_bytes = moved = 0
    try:
        pos = 0
        while True:
            chunk = text[pos:pos + window]
            last = pos + window >= text.size
            d.from_host(chunk)
            info = p.chunk_device(d.ptr, chunk.size, last)
            t0 = time.perf_counter()
            fi = f.format_device((p, d.ptr, chunk.size), p.device())
            wall += time.perf_counter() - t0
            for k in ms:
                ms[k] += fi[k]
            reads, out_bytes = reads + fi["n_records"], out_bytes + fi["out_bytes"]
            moved += fi["head_bytes"] + 2 * fi["seq_bytes"] + (fi["out_bytes"] + 15) // 16 * 16
            if last:
                break
            assert info["consumed"] > 0, "the window is smaller than one record"
            pos += info["consumed"]
    finally:
        d.free()
    gb = out_bytes / 1e9
    return dict(wall_s=wall, reads=reads, out_bytes=out_bytes, **ms, ms_per_gb={k: v / gb for k, v in ms.items()},
                gather_gbps=moved / (ms["ms_gather"] * 1e6) if ms["ms_gather"] else None)


def program(path, tmp, text_on_device):
    env = {k: v for k, v in os.environ.items() if k not in ("DBGK_TEXT", "DBGK_GUNZIP", "DBGK_TEST_HOOKS")}
    env["DBGK_GZ"] = "device"
    if text_on_device:
        env["DBGK_TEXT"] = "device"
    out = os.path.join(tmp, "out_%d.gz" % text_on_device)
    t0 = time.perf_counter()
    subprocess.run([os.path.join(ROOT, "dbg_assembly_amd", "bin", "clean_lowqual"), path, out, out + ".stat"], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    wall = time.perf_counter() - t0
    return {"wall_s": wall, "stat": open(out + ".stat").read(), "gz_bytes": os.path.getsize(out)}


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
    job = dict(reads=a.reads, program_reads=a.program_reads, read_len=READ_LEN, window_bytes=a.window, reps=a.reps)
    if capi.lib().dbgk_device_count() < 1:
        with open(a.out, "w") as f:
            json.dump({"job": job, "missing": FIGURES, "note": "no GPU on the machine this file was written on: nothing here is measured"}, f, indent=1)
            f.write("\n")
        print("no GPU: wrote the list of missing figures to", a.out)
        return
    text = make_text(a.reads)
    per = text.size // a.reads
    job["text_bytes"] = int(text.size)
    runs = {"old_compose_upload": [], "new_format": [], "program_host_text": [], "program_device_text": []}
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp, tempfile.TemporaryDirectory() as build:
        L = build_helper(build)
        path, small = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "reads_1m.fq")
        text.tofile(path)
        text[:a.program_reads * per].tofile(small)
        print("text written", file=sys.stderr, flush=True)
        with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(1, True) as p, capi.Formatter(1) as f:
            new_route(capi, g, p, f, text[:min(text.size, 64 << 20) // per * per], a.window)   # first touch of every buffer, not counted
            for _ in range(a.reps):   # interleaved, so that a drift of the machine meets every route
                runs["old_compose_upload"].append(old_route(capi, L, g, path))
                runs["new_format"].append(new_route(capi, g, p, f, text, a.window))
                print("run %d: %s" % (len(runs["new_format"]), {k: round(v[-1]["wall_s"], 3) for k, v in runs.items() if v}), file=sys.stderr, flush=True)
            copy_gbps = g.copy_bandwidth(2 << 30, 5)
        for r_old, r_new in zip(runs["old_compose_upload"], runs["new_format"]):
            assert r_old["reads"] == r_new["reads"] == a.reads and r_old["out_bytes"] == r_new["out_bytes"] == text.size
        program(small, tmp, True)   # first run of the binaries, not counted
        for _ in range(a.reps):
            runs["program_host_text"].append(program(small, tmp, False))
            runs["program_device_text"].append(program(small, tmp, True))
            print("program run %d: %.3f %.3f" % (len(runs["program_host_text"]), runs["program_host_text"][-1]["wall_s"],
                                                 runs["program_device_text"][-1]["wall_s"]), file=sys.stderr, flush=True)
        assert len({r["stat"] for k in ("program_host_text", "program_device_text") for r in runs[k]}) == 1, "the .stat files differ"
        for k in ("program_host_text", "program_device_text"):
            for r in runs[k]:
                del r["stat"]
    verdict = {"composition": verdict_of(runs["new_format"], runs["old_compose_upload"]),
               "program": verdict_of(runs["program_device_text"], runs["program_host_text"])}
    out = {"job": job, "runs": runs, "rule": "the slowest run of the new route against the fastest run of the old", "verdict": verdict,
           "copy_bandwidth_gbps": copy_gbps, "gather_over_copy": [r["gather_gbps"] / copy_gbps for r in runs["new_format"]],
           "bytes_counted": {"gather": "header, sequence and quality bytes read and the 16-byte vectors of text written; the offsets and records are not counted"},
           "notes": ["new_format wall_s is the time of the format_device calls alone: the batch lies on the device, as it does behind the cleaner",
                     "old_compose_upload wall_s is the loop of RecordBatch::write and the upload of its pieces; reading the records is not timed",
                     "the programs run with DBGK_GZ=device in both forms and read the same plain file from memory-backed storage"]}
    with open(a.out, "w") as f:
        json.dump(rounded(out), f, indent=1)
        f.write("\n")
    print(json.dumps(rounded({"verdict": verdict, "copy_bandwidth_gbps": copy_gbps, "ms_per_gb": [r["ms_per_gb"] for r in runs["new_format"]],
                              "gather_gbps": [r["gather_gbps"] for r in runs["new_format"]]})))


if __name__ == "__main__":
    main()
