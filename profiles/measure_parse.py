"""From the bytes of a FASTQ file to the device batch (bases, qualities, n + 1 offsets) on two routes, 10 M x 150 bp plain FASTQ
held in memory (and, for the host readers, in a file of the same bytes in the page cache):

  (a) today's routes   the project's own host readers (profiles/parse_old_route.cpp, built here with g++):
                       fill      RecordBatch::fill + the emptying of mismatched records + concat() of both planes per batch of 1 M
                                 records, as bin/clean_lowqual does, then the upload of both planes and the offsets;
                       chunked   ChunkedReadsFile with 16 reader threads, bases only, the sequences of a window copied back to back
                                 by the calling thread, then the upload of the bases and the offsets.
  (b) the new route    the upload of the text in windows (the bytes from `consumed` on presented again) + Parser.chunk_device per
                       window: with a quality plane against `fill`, without one against `chunked`.

Each route runs --reps times, interleaved.  Reported:
  1. the wall time of each route and its upload share; the project's rule decides whether the routes separate: the slowest run of
     the new route against the fastest of the old;
  2. the device time of the four phases (lines, states, scan, gather) summed over the windows, per GB of text;
  3. bytes read + written per second of the lines pass (the text read twice, the tile counts and the line table written) and of the
     gather (per plane the bytes read and the 16-byte vectors written), next to dbgk_measure_copy_bandwidth of the same run.
Writes profiles/parse_measure.json; without a GPU it lists the figures that are missing.  Reported, not gated.

    python profiles/measure_parse.py [--reads 10000000] [--window 268435456] [--reps 3]
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
OUT = os.path.join(ROOT, "profiles", "parse_measure.json")
FIGURES = ["old route fill wall_s (3 runs)", "old route chunked (16 threads, bases only) wall_s (3 runs)", "new route with qualities wall_s (3 runs)",
           "new route bases only wall_s (3 runs)", "routes_separate", "ms_lines, ms_states, ms_scan, ms_gather per GB of text",
           "lines pass GB/s (bytes read + written)", "gather GB/s (bytes read + written)", "copy_bandwidth GB/s of the same run"]
READ_LEN = 150
BATCH_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64)


def make_text(n, seed=1):
    """n records "@rNNNNNNNNN / 150 bases / + / 150 qualities" as one uint8 array"""
    rng = np.random.default_rng(seed)
    width = 11 + (READ_LEN + 1) + 2 + (READ_LEN + 1)
    text = np.empty((n, width), dtype=np.uint8)
    block = 1 << 20
    for a in range(0, n, block):
        b = min(n, a + block)
        t = text[a:b]
        t[:, 0], t[:, 1] = ord("@"), ord("r")
        idx = np.arange(a, b, dtype=np.int64)
        for d in range(9):
            t[:, 2 + d] = ord("0") + (idx // 10 ** (8 - d)) % 10
        t[:, 10] = 10
        t[:, 11:11 + READ_LEN] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (b - a, READ_LEN))]
        t[:, 11 + READ_LEN] = 10
        t[:, 12 + READ_LEN], t[:, 13 + READ_LEN] = ord("+"), 10
        t[:, 14 + READ_LEN:14 + 2 * READ_LEN] = rng.integers(35, 75, (b - a, READ_LEN), dtype=np.uint8)   # '@' among them
        t[:, 14 + 2 * READ_LEN] = 10
    return text.reshape(-1)


def build_helper(tmp):
    so = os.path.join(tmp, "parse_old_route.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "dbg_assembly_amd", "host"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "profiles", "parse_old_route.cpp"), "-o", so, "-lz", "-lpthread"], check=True)
    L = ctypes.CDLL(so)
    L.old_fill.restype = L.old_chunked.restype = ctypes.c_longlong
    L.old_fill.argtypes = [ctypes.c_char_p, BATCH_CB]
    L.old_chunked.argtypes = [ctypes.c_char_p, ctypes.c_int, BATCH_CB]
    return L


class Planes:
    """device buffers the old routes upload into"""

    def __init__(self, g, nbytes, reads):
        self.g, self.b, self.q, self.o = g, g.malloc(nbytes), g.malloc(nbytes), g.malloc((reads + 1) * 8)
        self.upload_s, self.reads, self.bases = 0.0, 0, 0

    def take(self, bases, quals, offsets, n, nb):
        from dbg_assembly_amd import capi
        t0 = time.perf_counter()
        assert nb <= self.b.nbytes and (n + 1) * 8 <= self.o.nbytes
        for dst, src, size in ((self.b, bases, nb), (self.q, quals, nb), (self.o, offsets, (n + 1) * 8)):
            if src and size:
                assert capi.lib().dbgk_memcpy_h2d(self.g._h, dst.ptr, ctypes.c_void_p(src), size) == 0
        self.upload_s += time.perf_counter() - t0
        self.reads += n
        self.bases += nb

    def free(self):
        for d in (self.b, self.q, self.o):
            d.free()


def old_route(L, g, path, which, threads=16):
    planes = Planes(g, 512 << 20, 4 << 20)
    try:
        cb = BATCH_CB(planes.take)
        t0 = time.perf_counter()
        n = L.old_fill(path.encode(), cb) if which == "fill" else L.old_chunked(path.encode(), threads, cb)
        wall = time.perf_counter() - t0
        assert n == planes.reads
        return {"wall_s": wall, "upload_s": planes.upload_s, "host_s": wall - planes.upload_s, "reads": planes.reads, "bases": planes.bases}
    finally:
        planes.free()


def new_route(capi, g, p, text, window, with_quals):
    d = g.malloc(window + 16)
    ms = {"ms_lines": 0.0, "ms_states": 0.0, "ms_scan": 0.0, "ms_gather": 0.0}
    upload = 0.0
    reads = bases = lines = windows = 0
    try:
        t0 = time.perf_counter()
        pos = 0
        while True:
            chunk = text[pos:pos + window]
            last = pos + window >= text.size
            t1 = time.perf_counter()
            d.from_host(chunk)
            upload += time.perf_counter() - t1
            info = p.chunk_device(d.ptr, chunk.size, last)
            for f in ms:
                ms[f] += info[f]
            reads, bases, lines, windows = reads + info["n_records"], bases + info["n_bases"], lines + info["n_lines"], windows + 1
            if last:
                break
            assert info["consumed"] > 0, "the window is smaller than one record"
            pos += info["consumed"]
        wall = time.perf_counter() - t0
    finally:
        d.free()
    gb = text.size / 1e9
    tiles = -(-text.size // capi.PARSE_TEXT_TILE)
    lines_bytes = 2 * text.size + 12 * tiles + 4 * lines
    gather_bytes = (2 if with_quals else 1) * (bases + (bases + 15) // 16 * 16)
    return dict(wall_s=wall, upload_s=upload, parse_s=wall - upload, reads=reads, bases=bases, windows=windows, **ms,
                ms_per_gb={f: v / gb for f, v in ms.items()}, lines_gbps=lines_bytes / (ms["ms_lines"] * 1e6) if ms["ms_lines"] else None,
                gather_gbps=gather_bytes / (ms["ms_gather"] * 1e6) if ms["ms_gather"] else None)


def rounded(x):
    if isinstance(x, float):
        return round(x, 4)
    if isinstance(x, dict):
        return {k: rounded(v) for k, v in x.items()}
    if isinstance(x, list):
        return [rounded(v) for v in x]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--window", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    job = dict(reads=a.reads, read_len=READ_LEN, window_bytes=a.window, reps=a.reps, chunked_threads=16, fill_batch_reads=1 << 20)
    if capi.lib().dbgk_device_count() < 1:
        with open(a.out, "w") as f:
            json.dump({"job": job, "missing": FIGURES, "note": "no GPU on the machine this file was written on: nothing here is measured"}, f, indent=1)
            f.write("\n")
        print("no GPU: wrote the list of missing figures to", a.out)
        return
    text = make_text(a.reads)
    job["text_bytes"] = int(text.size)
    runs = {"fill": [], "chunked": [], "new_with_quals": [], "new_bases_only": []}
    # the file of the host readers in memory where the system offers it; the helper elsewhere (such a place may not map code)
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp, tempfile.TemporaryDirectory() as build:
        L = build_helper(build)
        path = os.path.join(tmp, "reads.fq")
        text.tofile(path)
        with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(1, True) as pq, capi.Parser(1, False) as pb:
            new_route(capi, g, pq, text[:min(text.size, 64 << 20)], a.window, True)   # first touch of every buffer, not counted
            for _ in range(a.reps):   # interleaved, so that a drift of the machine meets every route
                runs["fill"].append(old_route(L, g, path, "fill"))
                runs["new_with_quals"].append(new_route(capi, g, pq, text, a.window, True))
                runs["chunked"].append(old_route(L, g, path, "chunked"))
                runs["new_bases_only"].append(new_route(capi, g, pb, text, a.window, False))
                print("run %d: %s" % (len(runs["fill"]), {k: round(v[-1]["wall_s"], 3) for k, v in runs.items()}), file=sys.stderr, flush=True)
            copy_gbps = g.copy_bandwidth(2 << 30, 5)
    for name in runs:
        assert len({(r["reads"], r["bases"]) for r in runs[name]}) == 1 and runs[name][0]["reads"] == a.reads, name
    verdict = {}
    for new, old in (("new_with_quals", "fill"), ("new_bases_only", "chunked")):
        slow_new, fast_old = max(r["wall_s"] for r in runs[new]), min(r["wall_s"] for r in runs[old])
        verdict[new + "_vs_" + old] = {"slowest_new_s": slow_new, "fastest_old_s": fast_old, "routes_separate": bool(slow_new < fast_old),
                                       "speedup_slowest_new_vs_fastest_old": fast_old / slow_new}
    out = {"job": job, "runs": runs, "rule": "the slowest run of the new route against the fastest run of the old; wall time with the uploads",
           "verdict": verdict, "copy_bandwidth_gbps": copy_gbps,
           "lines_over_copy": [r["lines_gbps"] / copy_gbps for r in runs["new_with_quals"]],
           "gather_over_copy": [r["gather_gbps"] / copy_gbps for r in runs["new_with_quals"]],
           "bytes_counted": {"lines": "the text read by k_parse_count and again by k_parse_lines, 12 bytes per tile (count, scan), 4 bytes per line",
                             "gather": "per plane the bytes read and the 16-byte vectors written"},
           "notes": ["ms_lines spans k_parse_count, the tile scan and k_parse_lines without the host round trip between them",
                     "the old routes read the file through the page cache (gzread of a plain file, pread); the new route starts from the same bytes in memory",
                     "old route `chunked`: the calling thread copies the sequences back to back; the programs pack them with several threads"]}
    with open(a.out, "w") as f:
        json.dump(rounded(out), f, indent=1)
        f.write("\n")
    print(json.dumps(rounded({"verdict": verdict, "copy_bandwidth_gbps": copy_gbps,
                              "ms_per_gb": [r["ms_per_gb"] for r in runs["new_with_quals"]],
                              "lines_gbps": [r["lines_gbps"] for r in runs["new_with_quals"]],
                              "gather_gbps": [r["gather_gbps"] for r in runs["new_with_quals"]]})))


if __name__ == "__main__":
    main()
