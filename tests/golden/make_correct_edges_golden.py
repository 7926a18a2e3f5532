"""Pin the corrector's edge scenarios (tests/correct_edge_cases.py) with the REAL reference program: run it on every pinned
scenario and write tests/golden/correct_edges/ -- cases.json and, per scenario, the reads (<name>.fa.gz), the reference's
<name>.correct.fa.gz (recompressed without a time stamp) and its <name>.correct.stat.  Tables of k <= 13 are committed
(<table>.cz + .cz.len, the format kmerfreq -b 1 writes; scenarios may share one); for k = 15, 16 and 17 the full table is
written to a temporary directory for the run only, and the tests rebuild it from the scenario's own specification.  The
unpinned scenarios (k = 1, k = 19, windows that start with a byte outside ACGTN) are never sent to the reference.

The fixtures are data; this script needs the reference only when it is run.  oracle/Makefile builds the binary
(`make -C oracle ref` -> oracle/_ref/ref_correct):

    python tests/golden/make_correct_edges_golden.py [oracle/_ref/ref_correct]
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
import correct_edge_cases as E  # noqa: E402
from make_correct_golden import BLOCK_BYTES, write_bytes  # noqa: E402

OUT = os.path.join(HERE, "correct_edges")
COMMIT_TABLE_MAX_K = 13


def write_table(path, T):
    """the .cz / .cz.len container of the raw table, one 1 MiB block at a time (the whole table is never held)"""
    nb = T.table_bytes()
    sparse = {}
    if not T.inverted:
        for at, blk in T.raw_blocks():
            sparse.setdefault(at // BLOCK_BYTES, []).append((at % BLOCK_BYTES, blk))
    empty = {}
    with open(path, "wb") as fz, open(path + ".len", "w") as fl:
        for b in range((nb + BLOCK_BYTES - 1) // BLOCK_BYTES):
            n = min(BLOCK_BYTES, nb - b * BLOCK_BYTES)
            if T.inverted:
                c = zlib.compress(T.raw_block(b * BLOCK_BYTES, n).tobytes())
            elif b in sparse:
                raw = np.zeros(n, dtype=np.uint8)
                for at, blk in sparse[b]:
                    raw[at:at + blk.size] = blk
                c = zlib.compress(raw.tobytes())
            else:
                if n not in empty:
                    empty[n] = zlib.compress(bytes(n))
                c = empty[n]
            fz.write(c)
            fl.write("%d\n" % len(c))


def ref_args(scn):
    o = scn.opts
    return ["-k", str(scn.k), "-t", "4", "-f", "2", "-m", str(o["m"]), "-c", str(o["c"]), "-x", str(o["x"]), "-n", str(o["n"]),
            "-r", str(o["r"])]


def run_reference(exe, scn, table_path, tmp):
    """-> (.correct.fa bytes, .correct.stat text, node-limit messages, Kmer_hifreq_num)"""
    rfile = os.path.join(tmp, scn.name + ".fa")
    open(rfile, "wb").write(E.reads_file(scn))
    with open(os.path.join(tmp, "reads.lib"), "w") as f:
        f.write(" %s \n" % rfile)
    r = subprocess.run([exe] + ref_args(scn) + [table_path, os.path.join(tmp, "reads.lib")], capture_output=True, text=True,
                       check=True, timeout=3600)
    fa = gzip.open(rfile + ".correct.fa.gz", "rb").read()
    stat = open(rfile + ".correct.stat").read()
    return fa, stat, r.stderr.count("node_vec_pos exceed Max_node_in_BB_tree"), int(r.stderr.split("Kmer_hifreq_num")[1].split()[0])


def main():
    exe = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "oracle", "_ref", "ref_correct"))
    only = sys.argv[2:]
    os.makedirs(OUT, exist_ok=True)
    meta, written = [], set()
    for scn in E.scenarios():
        if not scn.pinned:
            continue
        committed = scn.k <= COMMIT_TABLE_MAX_K
        entry = {"name": scn.name, "k": scn.k, "format": 2, "args": ref_args(scn), "reads": scn.name + ".fa.gz",
                 "table": scn.table_name + ".cz" if committed else None}
        if only and scn.name not in only:     # keep what an earlier run wrote
            old = {c["name"]: c for c in json.load(open(os.path.join(OUT, "cases.json")))}
            meta.append(old[scn.name])
            continue
        with tempfile.TemporaryDirectory() as tmp:
            tpath = os.path.join(OUT if committed else tmp, scn.table_name + ".cz")
            if tpath not in written:
                write_table(tpath, scn.table)
                written.add(tpath)
            fa, stat, hits, hif = run_reference(exe, scn, tpath, tmp)
        write_bytes(os.path.join(OUT, entry["reads"]), E.reads_file(scn), True)
        write_bytes(os.path.join(OUT, scn.name + ".correct.fa.gz"), fa, True)
        open(os.path.join(OUT, scn.name + ".correct.stat"), "w").write(stat)
        entry.update(node_limit_hits=hits, hifreq=hif)
        meta.append(entry)
        print(scn.name, "hits", hits, "hifreq", hif, flush=True)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(m) for m in meta) + "\n]\n")


if __name__ == "__main__":
    main()
