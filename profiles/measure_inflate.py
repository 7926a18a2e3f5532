"""The INFLATE stage measured against zlib on the host, one thread and 16 threads over members.

    python profiles/measure_inflate.py [--reads 10000000] [--window 268435456] [--reps 3] [--threads 16]

Writes profiles/inflate_measure.json.  Rule: three runs each, and the verdict is the slowest run of the new route against the fastest
run of the old one.  Text: 10 M x 150 bp FASTQ (as profiles/measure_parse.py makes it, 3.15 GB), in two framings:
  own     the project's level-2 members (Deflater, on the device)
  zlib6   zlib level 6 per piece of 65 280 bytes in BGZF framing, which is what bgzip writes
  device figures   upload + inflate with the text left on the device (Inflater.inflate without the download), the same plus download,
                   in windows of --window bytes of members; ms_decode, ms_resolve and ms_scan per GB of output; decoded symbols per
                   second; the decoders resident at once; the decode kernel's bytes read + written per second next to
                   dbgk_measure_copy_bandwidth of the same run
  baseline         zlib.decompress(member, wbits=31) over the members, in one thread and in --threads threads (the members are
                   independent and zlib releases the interpreter lock)
Without a GPU the script writes which figures are missing and measures nothing."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from measure_parse import READ_LEN, make_text, rounded  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "inflate_measure.json")
PIECE = 65280
HEAD = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0])
FIGURES = ["upload + inflate wall_s (3 runs)", "upload + inflate + download wall_s (3 runs)", "ms_decode, ms_resolve, ms_scan per GB of output",
           "decoded symbols per second", "resident decoders", "decode GB/s read + written", "copy_bandwidth GB/s of the same run",
           "zlib inflate wall_s, 1 thread and 16 threads (3 runs)"]


def zlib_members(text, threads):
    """zlib level 6 per piece, BGZF framing"""
    def one(a):
        piece = bytes(text[a:a + PIECE])
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = c.compress(piece) + c.flush()
        return HEAD + struct.pack("<H", len(raw) + 25) + raw + struct.pack("<II", zlib.crc32(piece), len(piece))
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range(0, text.size, PIECE)))


def split(buf):
    out, at = [], 0
    while at < len(buf):
        size = struct.unpack_from("<H", buf, at + 16)[0] + 1
        out.append(bytes(buf[at:at + size]))
        at += size
    return out


def host_runs(members, threads, reps):
    def some(lo):
        return sum(len(zlib.decompress(m, wbits=31)) for m in members[lo:lo + 64])
    res = {"one_thread": [], "threads": []}
    for _ in range(reps):
        t0 = time.perf_counter()
        n = sum(some(lo) for lo in range(0, len(members), 64))
        res["one_thread"].append(time.perf_counter() - t0)
        with ThreadPoolExecutor(threads) as ex:
            t0 = time.perf_counter()
            n2 = sum(ex.map(some, range(0, len(members), 64)))
            res["threads"].append(time.perf_counter() - t0)
        assert n == n2
    return res, n


def device_run(capi, z, windows, download):
    wall, ms, info_sum = 0.0, {f: 0.0 for f, _ in capi.InfTiming._fields_}, {"out_bytes": 0, "n_literals": 0, "n_matches": 0, "n_bad": 0, "n_members": 0}
    L = capi.lib()
    for w in windows:
        info = capi.InfInfo()
        t0 = time.perf_counter()
        rc = L.dbgk_inf_inflate(z._h, w.ctypes.data, w.size, 1, C.byref(info))
        if download:
            out = np.empty(info.out_bytes, dtype=np.uint8)
            rc = rc or L.dbgk_inf_results(z._h, out.ctypes.data, out.size)
        wall += time.perf_counter() - t0
        assert rc == 0 and info.consumed == w.size
        for f in info_sum:
            info_sum[f] += getattr(info, f)
        for f, v in z.timing().items():
            ms[f] += v
    return dict(wall_s=wall, **ms, **info_sum)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--window", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from dbg_assembly_amd import capi
    job = dict(reads=a.reads, read_len=READ_LEN, window_bytes=a.window, reps=a.reps, threads=a.threads, round_members=capi.INF_ROUND)
    if capi.lib().dbgk_device_count() < 1:
        with open(a.out, "w") as f:
            json.dump({"job": job, "missing": FIGURES, "note": "no GPU on the machine this file was written on: nothing here is measured"}, f, indent=1)
            f.write("\n")
        print("no GPU: wrote the list of missing figures to", a.out)
        return
    text = make_text(a.reads)
    framings = {}
    with capi.Deflater(2) as dz:
        own = []
        for lo in range(0, text.size, 1024 * PIECE):
            own += split(dz.deflate(text[lo:lo + 1024 * PIECE], last=False))
        framings["own"] = own
    framings["zlib6"] = zlib_members(text, a.threads)
    out = {"job": job, "rule": "the slowest run of the new route against the fastest run of the old, on the whole text", "text_bytes": int(text.size),
           "framings": {}}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        for name, members in framings.items():
            windows, cur, size = [], [], 0
            for m in members:
                if size + len(m) > a.window and cur:
                    windows.append(np.frombuffer(b"".join(cur), dtype=np.uint8))
                    cur, size = [], 0
                cur.append(m)
                size += len(m)
            windows.append(np.frombuffer(b"".join(cur), dtype=np.uint8))
            host, n = host_runs(members, a.threads, a.reps)
            assert n == text.size
            with capi.Inflater() as z:
                device_run(capi, z, windows[:1], True)   # first touch of every buffer, not counted
                left = [device_run(capi, z, windows, False) for _ in range(a.reps)]
                down = [device_run(capi, z, windows, True) for _ in range(a.reps)]
            assert all(r["n_bad"] == 0 and r["out_bytes"] == text.size for r in left + down)
            gb, packed = text.size / 1e9, sum(len(m) for m in members)
            r0 = left[0]
            symbols = r0["n_literals"] + r0["n_matches"]
            res = {"members": len(members), "packed_bytes": packed, "ratio": packed / text.size, "host_wall_s": host, "device_left_on_device": left,
                   "device_with_download": down,
                   "ms_per_gb": {f: [r[f] / gb for r in left] for f in ("ms_decode", "ms_resolve", "ms_scan")},
                   "symbols": symbols, "symbols_per_s": [symbols / (r["ms_decode"] * 1e-3) for r in left],
                   "resident_decoders": min(len(members), capi.INF_ROUND),
                   "decode_gbps": [(packed + 4 * symbols) / (r["ms_decode"] * 1e6) for r in left]}
            for route, runs in (("left_on_device", left), ("with_download", down)):
                slow = max(r["wall_s"] for r in runs)
                res["verdict_" + route] = {"slowest_new_s": slow, "fastest_one_thread_s": min(host["one_thread"]), "fastest_threads_s": min(host["threads"]),
                                           "beats_one_thread": bool(slow < min(host["one_thread"])), "beats_threads": bool(slow < min(host["threads"]))}
            out["framings"][name] = res
            print(name, rounded({k: v for k, v in res.items() if k.startswith("verdict") or k in ("ms_per_gb", "symbols_per_s")}), file=sys.stderr, flush=True)
        out["copy_bandwidth_gbps"] = g.copy_bandwidth(2 << 30, 5)
    for res in out["framings"].values():
        res["decode_share_of_copy_rate"] = [v / out["copy_bandwidth_gbps"] for v in res["decode_gbps"]]
    out["notes"] = ["the baseline is zlib.decompress per member through Python's zlib module; the 16 threads take 64 members at a time",
                    "resident decoders: the members of one round of the token area, one decoding lane each",
                    "decode_gbps counts the members' bytes read and the 4-byte tokens written"]
    with open(a.out, "w") as f:
        json.dump(rounded(out), f, indent=1)
        f.write("\n")
    print(json.dumps(rounded({n: {k: v for k, v in r.items() if k not in ("device_left_on_device", "device_with_download")} for n, r in out["framings"].items()}
                             | {"copy_gbps": out["copy_bandwidth_gbps"]})))


if __name__ == "__main__":
    main()
