"""The DEFLATE stage measured against single-threaded zlib at its default level, on the text the bin/ programs write.

    python profiles/measure_deflate.py [--reads 10000000] [--window 268435456] [--reps 3] [--baseline-bytes 536870912]

Writes profiles/deflate_measure.json.  Rule: three runs each, and the verdict is the slowest run of the new route against the fastest
run of the old one.  Text: 10 M x 150 bp FASTQ (as profiles/measure_parse.py makes it, 3.15 GB) and the FASTA a `.correct.fa` holds
for the same reads, in windows of 256 MiB, at every level with a Huffman code.
  device figures   upload + deflate + download per window (Deflater.deflate), deflate_device alone on a window that already lies on the
                   device, the device ms per phase (dbgk_gz_timing: the member launch by events, divided among match, CRC + histogram,
                   codes and encoding by the cycles its workgroups count; compaction: size scan + gather), bytes read + written per second next to
                   dbgk_measure_copy_bandwidth of the same run
  baseline         zlib's deflate at level 6 in one thread, fed in 1 MiB pieces as gzwrite feeds it, on a 512 MiB prefix of the same
                   text (enough: its rate does not depend on the length), scaled per GB
  size             output bytes over input bytes on that prefix: the stage, zlib -6 and zlib -1 over the whole prefix
  end to end       bin/clean_lowqual on 1 M reads with and without DBGK_GZ=device, wall clock, the same binary
Without a GPU the script writes which figures are missing and measures nothing."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from measure_parse import READ_LEN, make_text, rounded  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "deflate_measure.json")
FIGURES = ["upload + deflate + download wall_s (3 runs)", "deflate_device wall_s (3 runs)", "ms_members and its phases (match, crc + histogram, codes, encode), ms_compact per GB", "GB/s read + written",
           "copy_bandwidth GB/s of the same run", "zlib -6 single thread s per GB (3 runs)", "size ratios: stage, zlib -6, zlib -1",
           "bin/clean_lowqual wall_s with and without DBGK_GZ=device (3 runs)"]
TAIL = b"\tModifiedBaseNum: 0\tFinalReadLength: 150\tLeftEndTrim: 0\tRightEndTrim: 0\tIsDeleted: 0\n"


def fasta_of(fastq, n):
    """the two lines correct_error_reads writes per read, for the reads of make_text's FASTQ"""
    src = fastq.reshape(n, -1)
    tail = np.frombuffer(TAIL, dtype=np.uint8)
    out = np.empty((n, 10 + tail.size + READ_LEN + 1), dtype=np.uint8)
    out[:, :10] = src[:, :10]
    out[:, 0] = ord(">")
    out[:, 10:10 + tail.size] = tail
    out[:, 10 + tail.size:] = src[:, 11:11 + READ_LEN + 1]
    return out.reshape(-1)


def zlib_pass(text, level):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    t0, n = time.perf_counter(), 0
    for a in range(0, text.size, 1 << 20):
        n += len(c.compress(text[a:a + (1 << 20)]))
    n += len(c.flush())
    return time.perf_counter() - t0, n


def device_runs(capi, g, z, text, window):
    host = dev = 0.0
    out_bytes = 0
    ms = {f: 0.0 for f, _ in capi.GzTiming._fields_}
    d = g.malloc(window + 16)
    try:
        for a in range(0, text.size, window):
            chunk, last = text[a:a + window], a + window >= text.size
            t0 = time.perf_counter()
            out = z.deflate(chunk, last)
            host += time.perf_counter() - t0
            out_bytes += len(out)
            d.from_host(chunk)
            info = capi.GzInfo()
            t0 = time.perf_counter()
            rc = capi.lib().dbgk_gz_deflate_device(z._h, d.ptr, chunk.size, 1 if last else 0, info)
            dev += time.perf_counter() - t0
            assert rc == 0 and info.out_bytes == len(out)
            for f, v in z.timing().items():
                ms[f] += v
    finally:
        d.free()
    gb = text.size / 1e9
    moved = 2 * text.size + 3 * out_bytes   # the text staged once and read from LDS; slots zeroed and written; members read and written by the gather
    return dict(host_wall_s=host, device_wall_s=dev, out_bytes=out_bytes, ratio=out_bytes / text.size, **ms, ms_per_gb={f: v / gb for f, v in ms.items()},
                members_gbps=(text.size + 2 * out_bytes) / (ms["ms_members"] * 1e6), compact_gbps=2 * out_bytes / (ms["ms_compact"] * 1e6),
                bytes_moved=moved)


def end_to_end(text_1m, reps):
    exe = os.path.join(ROOT, "dbg_assembly_amd", "bin", "clean_lowqual")
    runs = {"zlib": [], "device": []}
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
        path = os.path.join(tmp, "reads.fq")
        text_1m.tofile(path)
        for _ in range(reps):
            for form in ("zlib", "device"):
                env = {k: v for k, v in os.environ.items() if k != "DBGK_GZ"}
                if form == "device":
                    env["DBGK_GZ"] = "device"
                t0 = time.perf_counter()
                r = subprocess.run([exe, path, os.path.join(tmp, "out.gz"), os.path.join(tmp, "out.stat")], env=env, capture_output=True, text=True, timeout=600)
                assert r.returncode == 0, r.stderr[-2000:]
                runs[form].append({"wall_s": time.perf_counter() - t0, "out_bytes": os.path.getsize(os.path.join(tmp, "out.gz"))})
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--window", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-bytes", type=int, default=512 << 20)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    job = dict(reads=a.reads, read_len=READ_LEN, window_bytes=a.window, reps=a.reps, baseline_bytes=a.baseline_bytes, levels=list(range(1, capi.GZ_MAX_LEVEL + 1)))
    if capi.lib().dbgk_device_count() < 1:
        with open(a.out, "w") as f:
            json.dump({"job": job, "missing": FIGURES, "note": "no GPU on the machine this file was written on: nothing here is measured"}, f, indent=1)
            f.write("\n")
        print("no GPU: wrote the list of missing figures to", a.out)
        return
    fastq = make_text(a.reads)
    texts = {"fastq": fastq, "fasta": fasta_of(fastq, a.reads)}
    out = {"job": job, "rule": "the slowest run of the new route against the fastest run of the old, per GB of text", "texts": {}}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        for name, text in texts.items():
            prefix = text[:min(text.size, a.baseline_bytes)]
            res = {"text_bytes": int(text.size), "prefix_bytes": int(prefix.size), "zlib6": [], "levels": {}}
            for _ in range(a.reps):
                s, n = zlib_pass(prefix, 6)
                res["zlib6"].append({"wall_s": s, "s_per_gb": s / (prefix.size / 1e9), "ratio": n / prefix.size})
            s, n = zlib_pass(prefix, 1)
            res["zlib1"] = {"wall_s": s, "ratio": n / prefix.size}
            for level in job["levels"]:
                with capi.Deflater(level) as z:
                    z.deflate(text[:min(text.size, 64 << 20)])   # first touch of every buffer, not counted
                    runs = [device_runs(capi, g, z, text, a.window) for _ in range(a.reps)]
                    on_prefix = len(z.deflate(prefix))
                gb = text.size / 1e9
                slow_new, fast_old = max(r["host_wall_s"] for r in runs) / gb, min(r["s_per_gb"] for r in res["zlib6"])
                res["levels"][str(level)] = {"runs": runs, "ratio_on_prefix": on_prefix / prefix.size,
                                             "size_over_zlib6": on_prefix / prefix.size / res["zlib6"][0]["ratio"],
                                             "size_over_zlib1": on_prefix / prefix.size / res["zlib1"]["ratio"],
                                             "verdict": {"slowest_new_s_per_gb": slow_new, "fastest_old_s_per_gb": fast_old,
                                                         "routes_separate": bool(slow_new < fast_old), "speedup": fast_old / slow_new}}
                print(name, level, rounded(res["levels"][str(level)]["verdict"]), file=sys.stderr, flush=True)
            out["texts"][name] = res
        out["copy_bandwidth_gbps"] = g.copy_bandwidth(2 << 30, 5)
    per_read = fastq.size // a.reads
    out["clean_lowqual_1m_reads"] = end_to_end(fastq[:min(a.reads, 1000000) * per_read], a.reps)
    out["notes"] = ["the baseline is zlib's deflate at level 6 through Python's zlib module, one thread, 1 MiB per call: the code gzwrite runs",
                    "size ratios are taken on the prefix, the stage in one call (members of 65 280 bytes, no history across them)",
                    "members_gbps counts the text read once and the slot zeroed and written; compact_gbps the members read and written"]
    with open(a.out, "w") as f:
        json.dump(rounded(out), f, indent=1)
        f.write("\n")
    print(json.dumps(rounded({n: {"zlib6_s_per_gb": [r["s_per_gb"] for r in t["zlib6"]], "zlib6_ratio": t["zlib6"][0]["ratio"], "zlib1_ratio": t["zlib1"]["ratio"],
                                  "levels": {lv: dict(v["verdict"], ratio=v["ratio_on_prefix"], size_over_zlib6=v["size_over_zlib6"],
                                                      ms_per_gb=v["runs"][0]["ms_per_gb"], members_gbps=[r["members_gbps"] for r in v["runs"]],
                                                      compact_gbps=[r["compact_gbps"] for r in v["runs"]],
                                                      device_wall_s=[r["device_wall_s"] for r in v["runs"]]) for lv, v in t["levels"].items()}}
                              for n, t in out["texts"].items()} | {"copy_gbps": out["copy_bandwidth_gbps"],
                                                                   "clean_lowqual": {k: [r["wall_s"] for r in v] for k, v in out["clean_lowqual_1m_reads"].items()}})))


if __name__ == "__main__":
    main()
