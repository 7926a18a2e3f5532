"""GPU steps of tests/test_format_gpu.py, each run in a child process of its own under a time limit:
    python tests/format_gpu_steps.py crafted | device_input | chain | states
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
import format_cases as FC  # noqa: E402
import format_restatement as FR  # noqa: E402
from parse_gpu_steps import fetch, status_of  # noqa: E402


def check(f, g, info, want, name):
    """the text of the last call against the restatement: the counters, results(), and the whole 16-byte vectors where they lie
    (the zero pad included)"""
    text, want_info = want
    assert {k: info[k] for k in FR.COUNTERS} == want_info, (name, info, want_info)
    assert f.info == info
    ptr, n = f.device()
    assert n == len(text) and ptr and ptr % 16 == 0, name
    assert f.results() == text, (name, "results")
    vec, plane = fetch(g, ptr, -(-n // 16) * 16), FR.vectors(text)
    assert np.array_equal(vec, plane), (name, int(np.flatnonzero(vec != plane)[0]))
    if not n:
        assert info["ms_gather"] == 0
    return {k: info[k] for k in FR.COUNTERS}


def formatters(capi):
    """one handle per (format, marker), each used for every case that asks for it, in the order of the cases"""
    made = {}

    def get(fmt, marker):
        if (fmt, marker) not in made:
            made[fmt, marker] = capi.Formatter(fmt, marker)
        return made[fmt, marker]
    return made, get


def crafted():
    from dbg_assembly_amd import capi
    cases = FC.cases()
    for tag in ("fastq", "fasta"):
        assert FC.covers_every_residue(cases["sweep_0_100_" + tag])
    res = {}
    made, get = formatters(capi)
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        try:
            for name, c in cases.items():
                f = get(c["fmt"], c["marker"])
                info = f.format(c["text"], c["recs"], c["bases"], c["quals"], c["offsets"], c["suffixes"])
                res[name] = check(f, g, info, FC.expected(c), name)
            # the suffixes as a plane of the caller's own, and a plane of empty suffixes
            c = cases["sweep_0_100_fastq"]
            off = np.zeros(len(c["suffixes"]) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(s) for s in c["suffixes"]])
            f = get(c["fmt"], c["marker"])
            check(f, g, f.format(c["text"], c["recs"], c["bases"], c["quals"], c["offsets"], (np.frombuffer(b"".join(c["suffixes"]), np.uint8), off)),
                  FC.expected(c), "suffix plane")
            c = cases["first_record_ends_at_T+0_fasta"]
            f = get(c["fmt"], c["marker"])
            check(f, g, f.format(c["text"], c["recs"], c["bases"], c["quals"], c["offsets"], [b""] * len(c["recs"])), FC.expected(c), "empty suffixes")
        finally:
            for f in made.values():
                f.close()
    res["handles"] = len(made)
    return res


def place(g, data, front, fill, room=80):
    """data inside a larger device buffer filled with `fill`, at byte `front` (a multiple of 16) -> (buffer, host image)"""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    size = front + data.size + room
    size += -size % 16
    host = np.frombuffer((fill * size)[:size], dtype=np.uint8).copy()
    host[front:front + data.size] = data.view(np.uint8)
    d = g.malloc(size)
    d.from_host(host)
    return d, host


def device_input():
    """format_device on text, records, planes and offsets that lie inside larger device buffers whose every other byte is a newline, a
    marker or another non-zero byte: the text is the one of the stated ranges alone, and no input is written"""
    from dbg_assembly_amd import capi
    cases = FC.cases()
    res = {}
    made, get = formatters(capi)
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        try:
            for name, front in (("sweep_0_100_fastq", 16), ("sweep_0_100_fasta", 4096 + 48), ("header_ends_the_text_3_fastq", 32),
                                ("header_ends_the_text_2_fasta", 160), ("marker_3e_fasta", 64), ("run_of_3T_emptied_records_fastq", 48),
                                ("empty_fastq", 16)):
                c = cases[name]
                n = len(c["recs"])
                bufs = [place(g, c["text"], front, b"\n@>"), place(g, c["recs"].view(np.uint8), 16, b"\x07"),
                        place(g, c["bases"], front, b"\nA>"), place(g, c["offsets"].view(np.uint8), 32, b"\xff")]
                if c["quals"] is not None:
                    bufs.append(place(g, c["quals"], front, b"\nI@"))
                try:
                    f = get(c["fmt"], c["marker"])
                    planes = (bufs[2][0].ptr + front, bufs[4][0].ptr + front if c["quals"] is not None else None, bufs[3][0].ptr + 32, n)
                    info = f.format_device((bufs[0][0].ptr + front, len(c["text"]), bufs[1][0].ptr + 16), planes, c["suffixes"])
                    res[name] = check(f, g, info, FC.expected(c), name)
                    res[name]["tail"] = len(c["text"]) % 16
                    for d, host in bufs:
                        assert np.array_equal(d.to_host(np.uint8, host.size), host), (name, "an input was written")
                finally:
                    for d, _ in bufs:
                        d.free()
        finally:
            for f in made.values():
                f.close()
    assert {v["tail"] for v in res.values()} - {0}
    return res


def lowqual_suffixes(blocks, lens, min_len):
    """the annotation bin/clean_lowqual appends to every header (host/clean_lowqual.cpp), from the device's blocks and the lengths
    of the reads after the parser's emptying"""
    out = []
    for b, n in zip(blocks, lens):
        s = "    RQ: " + ("%.17g" % (float(b["error_sum"]) / n * 100) if n else "-nan") + "%"
        kept = n
        if b["trimmed"]:
            s += "  TrimLowQual"
            kept = int(b["length"]) if b["start"] >= 1 else 0
        if kept < min_len:
            s += "  FilterShort"
        out.append(s.encode("latin-1"))
    return out


def chain():
    """three CLEAN inputs through Parser -> Cleaner.lowqual_device -> compact -> Formatter where they lie: the text is the file the
    reference wrote; the formatter's output parsed again where it lies is the compact batch; deflated where it lies and inflated by
    zlib it is the same text"""
    from dbg_assembly_amd import capi
    import clean_restatement as CR
    res = {}
    wanted = {"mixed.fq", "reads.fq", "phred64.fq"}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(FC.FASTQ, True) as p, capi.Parser(FC.FASTQ, True) as p2, \
            capi.Cleaner() as c, capi.Formatter(FC.FASTQ) as f, capi.Deflater() as z:
        for case in CR.golden_cases(FC.CLEAN):
            if case["program"] != "clean_lowqual" or case["input"] not in wanted:
                continue
            o = CR.case_options(case)
            text = open(os.path.join(FC.CLEAN, case["input"]), "rb").read()
            d_text, _ = place(g, text, 0, b"\n", room=16)
            try:
                info = p.chunk_device(d_text.ptr, len(text))
                d_b, d_q, _, n, _ = p.device()
                _, _, offsets, recs = p.results()
                blocks = c.lowqual_device(d_b, d_q, offsets, o["-e"], o["-q"])
                c.compact(o["-r"])
                sufs = lowqual_suffixes(blocks, np.diff(offsets.astype(np.int64)), o["-r"])
                fi = f.format_device(p, c.compact_device(), sufs)   # the parser's records and the text of its chunk, where they lie
                want = CR.expected_outputs(FC.CLEAN, case)["out"].encode("latin-1")
                got = f.results()
                assert got == want, (case["name"], "the text differs from the reference's file")
                cb, cq, coff = c.compact_to_host()
                heads = [text[int(r["head_pos"]):int(r["head_pos"]) + int(r["head_len"])] for r in recs]
                check(f, g, fi, FR.format_batch(FC.FASTQ, text, recs, cb, cq, coff, sufs), case["name"])
                # the text parsed again where it lies: the compact batch and the annotated headers
                d_out, n_out = f.device()
                back = p2.chunk_device(d_out, n_out)
                b2, q2, o2, r2 = p2.results()
                assert back["n_records"] == n and back["ignored_lines"] == 0 and back["mismatched"] == 0, case["name"]
                assert np.array_equal(o2, coff) and np.array_equal(b2, cb) and np.array_equal(q2, cq), case["name"]
                assert [got[int(r["head_pos"]):int(r["head_pos"]) + int(r["head_len"])] for r in r2] == [h + s for h, s in zip(heads, sufs)]
                # ... and deflated where it lies
                assert gzip.decompress(z.deflate_device(d_out, n_out)) == want, case["name"]
                res[case["name"]] = {"input": case["input"], "records": n, "mismatched": info["mismatched"], "out_bytes": fi["out_bytes"]}
            finally:
                d_text.free()
    assert {v["input"] for v in res.values()} == wanted
    return res


def states():
    from dbg_assembly_amd import capi
    L = capi.lib()
    res = {}
    h = ctypes.c_void_p()
    res["format_3"] = L.dbgk_fmt_create(3, 0, 0, ctypes.byref(h))
    res["marker_256"] = L.dbgk_fmt_create(1, 256, 0, ctypes.byref(h))
    c = FC.build(FC.FASTQ, [b"@a", b"@bc"], [b"ACGT", b"AC"])
    ca = FC.build(FC.FASTA, [b">a", b">bc"], [b"ACGT", b"AC"])
    n = 2
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Formatter(FC.FASTQ) as fq, capi.Formatter(FC.FASTA) as fa, \
            capi.Parser(FC.FASTQ, True) as p:
        res["results_before_a_call"] = status_of(fq.results)
        res["device_before_a_call"] = status_of(fq.device)
        res["recs_of_a_parser_before_a_chunk"] = L.dbgk_parse_recs_device(p._h, ctypes.byref(h))
        res["text_of_a_parser_before_a_chunk"] = L.dbgk_parse_text_device(p._h, ctypes.byref(h), ctypes.byref(ctypes.c_uint64()))
        res["fastq_without_a_quality_plane"] = status_of(lambda: fq.format(c["text"], c["recs"], c["bases"], None, c["offsets"]))
        res["fasta_with_a_quality_plane"] = status_of(lambda: fa.format(c["text"], c["recs"], c["bases"], c["quals"], c["offsets"]))
        bufs = {k: place(g, v, 16, b"\n")[0] for k, v in (("text", c["text"]), ("recs", c["recs"].view(np.uint8)), ("bases", c["bases"]),
                                                           ("quals", c["quals"]), ("off", c["offsets"].view(np.uint8)))}
        at = {k: d.ptr + 16 for k, d in bufs.items()}

        def dev(fmt=fq, n_text=len(c["text"]), sufs=None, n_rec=n, **moved):
            a = dict(at, **moved)
            return status_of(lambda: fmt.format_device((a["text"], n_text, a["recs"]), (a["bases"], a["quals"] if fmt is fq else None, a["off"], n_rec), sufs))
        res["fastq_without_a_quality_plane_device"] = status_of(lambda: fq.format_device((at["text"], len(c["text"]), at["recs"]),
                                                                                          (at["bases"], None, at["off"], n)))
        res["fasta_with_a_quality_plane_device"] = status_of(lambda: fa.format_device((at["text"], len(c["text"]), at["recs"]),
                                                                                       (at["bases"], at["quals"], at["off"], n)))
        res["misaligned_text"] = dev(text=at["text"] + 4)
        res["misaligned_bases"] = dev(bases=at["bases"] + 8)
        res["misaligned_quals"] = dev(quals=at["quals"] + 1)
        res["n_text_2_to_the_31"] = dev(n_text=1 << 31)
        res["n_2_to_the_31"] = dev(n_rec=1 << 31)
        res["results_after_refused_calls"] = status_of(fq.results)
        res["good_call"] = dev()
        assert fq.results() == FC.expected(c)[0]
        d_out, _ = fq.device()
        res["own_output_as_text"] = dev(text=d_out)
        res["own_output_as_bases"] = dev(bases=d_out)
        res["own_output_as_quals"] = dev(quals=d_out)
        res["results_after_refused_input"] = status_of(fq.results)
        # found on the device: a header that leaves the text, offsets that decrease
        res["header_leaves_the_text"] = dev(n_text=len(c["text"]) - 2)   # (the last header ends at byte 6 of the 7)
        res["results_after_a_header_that_leaves_the_text"] = status_of(fq.results)
        res["header_ends_with_the_text"] = dev(n_text=len(c["text"]) - 1)
        bad = c["offsets"].copy()
        bad[1], bad[2] = bad[2], bad[1] - 1
        bufs["bad"] = place(g, bad.view(np.uint8), 16, b"\n")[0]
        res["decreasing_offsets_device"] = dev(off=bufs["bad"].ptr + 16)
        res["decreasing_offsets_host"] = status_of(lambda: fq.format(c["text"], c["recs"], c["bases"], c["quals"], bad))
        res["results_after_decreasing_offsets"] = status_of(fq.results)
        res["decreasing_suffix_offsets"] = status_of(lambda: fq.format(c["text"], c["recs"], c["bases"], c["quals"], c["offsets"],
                                                                        (np.zeros(4, np.uint8), np.array([0, 3, 2], dtype=np.uint64))))
        res["suffix_offsets_from_1"] = status_of(lambda: fq.format(c["text"], c["recs"], c["bases"], c["quals"], c["offsets"],
                                                                    (np.zeros(4, np.uint8), np.array([1, 2, 3], dtype=np.uint64))))
        res["no_records"] = dev(n_rec=0)
        assert fq.results() == b"" and fq.device()[1] == 0
        res["capacity_below_the_text"] = L.dbgk_fmt_results(fq._h, None, 0) if dev() == capi.OK else -100
        res["fasta_good_call"] = status_of(lambda: fa.format(ca["text"], ca["recs"], ca["bases"], None, ca["offsets"]))
        assert fa.results() == FC.expected(ca)[0]
        # the parser's records where they lie
        info = p.chunk_device(at["text"], 0)
        res["recs_of_a_parser_after_a_chunk"] = L.dbgk_parse_recs_device(p._h, ctypes.byref(h))
        n_text = ctypes.c_uint64(7)
        res["text_of_a_parser_after_a_chunk"] = L.dbgk_parse_text_device(p._h, ctypes.byref(h), ctypes.byref(n_text))
        assert h.value == at["text"] and n_text.value == 0
        assert info["n_records"] == 0
        for d in bufs.values():
            d.free()
    return res


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "device_input": device_input, "chain": chain, "states": states}[sys.argv[1]]()))
