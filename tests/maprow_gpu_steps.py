"""GPU steps of tests/test_maprow_gpu.py, each run in a child process of its own under a time limit:
    python tests/maprow_gpu_steps.py crafted | states | chain
Prints one JSON line of findings; exits non-zero on a mismatch."""
import ctypes
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_restatement as MR  # noqa: E402
import maprow_cases as MC  # noqa: E402
import maprow_restatement as RR  # noqa: E402
from parse_gpu_steps import fetch, status_of  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "map_cases")


def sides_of(case):
    return [(s["text"], s["recs"], s["bases"] if s["bases"] is not None else np.zeros(0, dtype=np.uint8), s["offsets"], s["hits"]) for s in case["sides"]]


def check_streams(w, g, want, name):
    """the three streams of the last call against the restatement: the counters, the bytes, and the whole 16-byte vectors on the device
    with the zero pad"""
    info = w.info
    assert info["counters"] == want["counters"], (name, info, want["counters"])
    assert info["unprintable"] == want["unprintable"], (name, info)
    assert info["stream_bytes"] == [len(s) for s in want["streams"]], (name, info["stream_bytes"], [len(s) for s in want["streams"]])
    for s, text in enumerate(want["streams"]):
        got = w.results(s)
        if got != text:
            at = next((k for k in range(min(len(got), len(text))) if got[k] != text[k]), min(len(got), len(text)))
            raise AssertionError((name, "stream %d differs at byte %d" % (s, at), got[max(0, at - 60):at + 40], text[max(0, at - 60):at + 40]))
        ptr, n = w.device(s)
        assert n == len(text) and ptr and ptr % 16 == 0, (name, s)
        padded = -(-n // 16) * 16
        image = np.zeros(padded, dtype=np.uint8)
        image[:n] = np.frombuffer(text, dtype=np.uint8)
        assert np.array_equal(fetch(g, ptr, padded), image), (name, s, "the pad behind the stream")
    if not any(want["streams"]):
        assert info["ms_write"] == 0
    return {"n": info["n"], "counters": info["counters"], "stream_bytes": info["stream_bytes"], "unprintable": info["unprintable"]}


def crafted():
    """every crafted batch through dbgk_maprow_rows, one handle per mode and delimiter set, in the order of the cases -- a handle sees
    large and small batches in turn"""
    from dbg_assembly_amd import capi
    res, writers = {}, {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        try:
            for name, case in MC.cases().items():
                key = (case["mode"], case["delims"], case["min_len"])
                if key not in writers:
                    writers[key] = capi.RowWriter(case["mode"], case["delims"], case["min_len"])
                w = writers[key]
                w.set_contigs(case["names"], case["lengths"])
                w.rows(sides_of(case))
                res[name] = check_streams(w, g, RR.expected(case), name)
        finally:
            for w in writers.values():
                w.close()
    return res


def states():
    from dbg_assembly_amd import capi
    res = {}
    c = MC.cases()
    reads, pair = c["reads_classes"], c["pair_classes"]
    with capi.RowWriter(capi.MAPROW_READS, b">@ \t\n", 20) as w, capi.RowWriter(capi.MAPROW_PAIR, b"@ \t", 30) as wp, \
            capi.Mapper(k=21, s=3, r=30, second_alignment=True) as m:
        res["results_before_a_call"] = status_of(lambda: w.results(0))
        res["device_before_a_call"] = status_of(lambda: w.device(0))
        res["rows_before_set_contigs"] = status_of(lambda: w.rows(sides_of(reads)))
        w.set_contigs(reads["names"], reads["lengths"])
        wp.set_contigs(pair["names"], pair["lengths"])
        res["rows_device_before_take_hits"] = status_of(lambda: w.rows_device([(None, 0, None, None, None)], 0))
        res["take_hits_before_a_batch"] = status_of(lambda: w.take_hits(0, m))
        res["hits_device_before_a_batch"] = status_of(m.hits_device)
        res["take_hits_side_2"] = status_of(lambda: w.take_hits(2, m))
        res["good_call"] = status_of(lambda: w.rows(sides_of(reads)))
        res["stream_3"] = status_of(lambda: w.device(3))
        info = capi.MapRowInfo()
        res["capacity_too_small"] = capi.lib().dbgk_maprow_results(w._h, 0, (ctypes.c_char * 8)(), 8)
        res["results_after_a_refused_capacity"] = status_of(lambda: w.results(0))

        def with_hit(case, **fields):
            side = dict(case["sides"][0], hits=case["sides"][0]["hits"].copy())
            for f, v in fields.items():
                side["hits"][0, 0][f] = v
            return [(side["text"], side["recs"], side["bases"] if side["bases"] is not None else np.zeros(0, dtype=np.uint8), side["offsets"], side["hits"])] + \
                sides_of(case)[1:]
        res["contig_outside_the_table"] = status_of(lambda: w.rows(with_hit(reads, contig=len(reads["names"]))))
        res["results_after_a_refused_batch"] = status_of(lambda: w.results(0))
        res["negative_coordinate"] = status_of(lambda: w.rows(with_hit(reads, contig_start=-5)))
        res["align_len_0"] = status_of(lambda: w.rows(with_hit(reads, align_len=0)))
        res["more_mismatches_than_bases"] = status_of(lambda: w.rows(with_hit(reads, mismatches=31)))
        res["pair_contig_outside_the_table"] = status_of(lambda: wp.rows(with_hit(pair, contig=99)))
        bad = dict(reads["sides"][0], recs=reads["sides"][0]["recs"].copy())
        bad["recs"][3]["head_len"] = len(bad["text"])
        res["header_leaves_the_text"] = status_of(lambda: w.rows([(bad["text"], bad["recs"], bad["bases"], bad["offsets"], bad["hits"])]))
        off = reads["sides"][0]["offsets"].copy()
        off[2] = off[1] - 1
        res["decreasing_offsets"] = status_of(lambda: w.rows([(reads["sides"][0]["text"], reads["sides"][0]["recs"], reads["sides"][0]["bases"], off,
                                                                 reads["sides"][0]["hits"])]))
        res["one_side_for_pair"] = capi.lib().dbgk_maprow_rows(wp._h, None, 1, ctypes.byref(info))
        res["good_call_again"] = status_of(lambda: w.rows(sides_of(reads)))
        assert w.results(1) == RR.expected(reads)["streams"][1]
        res["pair_good_call"] = status_of(lambda: wp.rows(sides_of(pair)))
        assert wp.results(2) == RR.expected(pair)["streams"][2]
        res["set_contigs_drops_the_text"] = (w.set_contigs(reads["names"], reads["lengths"]), status_of(lambda: w.results(0)))[1]
    return res


def golden_cases():
    return json.load(open(os.path.join(GOLDEN, "cases.json")))


def chain():
    """Parser -> Mapper.map_device(keep=True) -> take_hits -> rows_device on the inputs of tests/golden/map_cases, a reads file (or a pair
    of files) as one chunk, against the files the reference wrote; stream 0 deflated where it lies and inflated again by gzip"""
    from dbg_assembly_amd import capi
    res = {}
    for case in golden_cases():
        P = MR.params_of(case["args"])
        ids, contigs = MR.read_contig_file(os.path.join(GOLDEN, case["contigs"]), P.l)
        want = MR.expected_outputs(GOLDEN, case)
        files = MR.read_lib_file(os.path.join(GOLDEN, case["lib"]))
        pair = case["program"] == "map_pair"
        mode = capi.MAPROW_PAIR if pair else capi.MAPROW_READS
        delims = (b"@ \t" if P.fmt == 1 else b"> \t") if pair else b">@ \t\n"
        groups = list(zip(files[0::2], files[1::2])) if pair else [(f,) for f in files]
        with capi.Mapper(k=P.k, s=P.s, r=P.r, identity=P.i, second_alignment=not pair) as m, capi.RowWriter(mode, delims, P.r) as w, \
                capi.Deflater() as z:
            m.set_contigs(contigs)
            w.set_contigs([q.encode("latin-1") for q in ids], [len(q) for q in contigs])
            for group in groups:
                parsers = [capi.Parser(P.fmt) for _ in group]
                try:
                    n = None
                    for s, (f, p) in enumerate(zip(group, parsers)):
                        text = "\n".join(MR.open_text(os.path.join(GOLDEN, f))).encode("latin-1") + b"\n"
                        info = p.chunk(text)
                        assert info["ignored_lines"] == 0 and (n is None or n == info["n_records"]), (case["name"], f, info)
                        n = info["n_records"]
                        d_b, _, d_o, _, nb = p.device()
                        assert m.map_device(d_b, d_o, n, nb, info["max_len"], keep=True) is None
                        assert m.hits_device()[1] == n
                        w.take_hits(s, m)
                    info = w.rows_device(parsers, n)
                    got = RR.files_of(mode, [w.results(s) for s in range(3)], info["counters"])
                    for suffix, data in got.items():
                        assert data.decode("latin-1") == want[os.path.basename(group[0]) + suffix], (case["name"], group[0], suffix)
                    ptr, nbytes = w.device(0)
                    members = z.deflate_device(ptr, nbytes)
                    assert gzip.decompress(members) == w.results(0), (case["name"], "stream 0 deflated in place")
                    res["%s:%s" % (case["name"], os.path.basename(group[0]))] = {"n": n, "counters": info["counters"], "stream_bytes": info["stream_bytes"],
                                                                               "members": z.info["n_members"]}
                finally:
                    for p in parsers:
                        p.close()
    return res


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "states": states, "chain": chain}[sys.argv[1]]()))
