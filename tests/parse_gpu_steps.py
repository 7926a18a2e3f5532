"""GPU steps of tests/test_parse_gpu.py, each run in a child process of its own under a time limit:
    python tests/parse_gpu_steps.py crafted | many | chunking | device_input | lowqual | graph | states
Prints one JSON line of findings; exits non-zero on a mismatch."""
import ctypes
import gzip
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parse_cases as PC  # noqa: E402
import parse_restatement as PR  # noqa: E402

BIG = 60000   # lines from which a crafted case belongs to the step `many`


def fetch(g, ptr, nbytes):
    from dbg_assembly_amd import capi
    out = np.full(max(nbytes, 1), 0xAA, dtype=np.uint8)
    if nbytes:
        assert capi.lib().dbgk_memcpy_d2h(g._h, out.ctypes.data, ctypes.c_void_p(ptr), nbytes) == 0
    return out[:nbytes]


def check(p, g, info, want, name):
    """the batch of the last chunk against the restatement: every counter and `consumed`, the whole 16-byte vectors of both planes
    (the pad included), the offsets, the records"""
    assert {f: info[f] for f in PR.COUNTERS} == want["info"], (name, info, want["info"])
    bases, quals, offsets, recs = p.results()
    d_b, d_q, d_o, n, nb = p.device()
    assert (n, nb) == (len(want["records"]), int(want["offsets"][-1])) and d_b % 16 == 0 and d_o % 8 == 0, name
    assert (d_q is not None) == (want["quals"] is not None), name
    assert np.array_equal(offsets, want["offsets"]), (name, "offsets")
    assert recs.tobytes() == want["recs"].tobytes(), (name, "records")
    for ptr, got, plane, what in ((d_b, bases, want["bases"], "bases"), (d_q, quals, want["quals"], "quals")):
        if plane is None:
            assert got is None
            continue
        vec = fetch(g, ptr, plane.size)
        assert np.array_equal(vec, plane), (name, what, int(np.flatnonzero(vec != plane)[0]))
        assert np.array_equal(got, plane[:nb]), (name, what)
    if not nb:
        assert info["ms_gather"] == 0
    return {f: info[f] for f in ("n_records", "n_lines", "ignored_lines", "n_bases", "mismatched")}


def run_cases(cases):
    """every case with last 1 and 0, a FASTQ text with and without a quality plane -> the counters of (last, no qualities), and
    the restatement's batches"""
    from dbg_assembly_amd import capi
    res, wants = {}, {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(PC.FASTQ) as fq, capi.Parser(PC.FASTQ, True) as fqq, \
            capi.Parser(PC.FASTA) as fa:
        for name, (fmt, text) in cases.items():
            for with_quals in ((False, True) if fmt == PC.FASTQ else (False,)):
                p = fa if fmt == PC.FASTA else (fqq if with_quals else fq)
                for last in (True, False):
                    want = PR.parse(text, fmt, with_quals, last)
                    got = check(p, g, p.chunk(text, last), want, (name, with_quals, last))
                    wants[name, with_quals, last] = want
                    if last and not with_quals:
                        res[name] = got
    return res, wants


def crafted():
    cases = {k: v for k, v in PC.cases().items() if v[1].count(b"\n") < BIG}
    res, wants = run_cases(cases)
    for tag, total in PC.TOTALS.items():
        for with_quals in (False, True):
            assert wants["total_" + tag, with_quals, True]["info"]["n_bases"] == total
    w = wants["all_emptied", True, True]["info"]
    assert w["n_bases"] == 0 and w["mismatched"] == w["n_records"] == 300
    assert wants["line_of_3T_and_more", True, True]["info"]["max_len"] == 3 * PC.T + 100
    # every residue of source and destination position mod 16, every pair of them mod 4, for both planes
    w = wants["lengths_0_100", True, True]
    dst, lens = w["offsets"][:-1].astype(np.int64), np.diff(w["offsets"].astype(np.int64))
    for field in ("seq_pos", "qual_pos"):
        src, d = w["recs"][field].astype(np.int64)[lens > 0], dst[lens > 0]
        assert set((src % 16).tolist()) == set(range(16)) and set((d % 16).tolist()) == set(range(16)), field
        assert {(int(a), int(b)) for a, b in zip(src % 4, d % 4)} == {(a, b) for a in range(4) for b in range(4)}, field
    assert set(lens.tolist()) == set(range(101))
    res["lengths_0_100_residues"] = "all"
    return res


def many():
    """about 70 000 lines that all begin with the marker, in every phase: the map scan crosses many workgroups; and more lines than
    one round of the spine takes"""
    cases = {k: v for k, v in PC.cases().items() if v[1].count(b"\n") >= BIG}
    assert len(cases) == 7
    return run_cases(cases)[0]


def chunking():
    """one text of a few records through ONE handle: cut at its first and last byte and at every byte of its second record; the
    batches of the two chunks, concatenated, are the batch of the whole text, and every `consumed` is the restatement's"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(3)
    text = b"junk\n" + PC.fastq(rng, [20, 26, 0, 31])
    second = text.index(b"@r1\n")
    cuts = sorted({1, len(text)} | set(range(second, text.index(b"@r2\n") + 1)))
    assert len(cuts) <= 100
    res = {"cuts": len(cuts), "consumed_0": 0}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(PC.FASTQ, True) as p:
        whole = PR.parse(text, PC.FASTQ, True)
        check(p, g, p.chunk(text), whole, "whole")
        for cut in cuts:
            first = text[:cut]
            info = p.chunk(first, last=False)
            want = PR.parse(first, PC.FASTQ, True, last=False)
            check(p, g, info, want, ("first", cut))
            b1, q1, o1, r1 = p.results()
            res["consumed_0"] += info["consumed"] == 0 and info["n_records"] == 0
            rest = text[info["consumed"]:]
            info2 = p.chunk(rest, last=True)
            check(p, g, info2, PR.parse(rest, PC.FASTQ, True, last=True), ("rest", cut))
            b2, q2, o2, r2 = p.results()
            nb = int(whole["offsets"][-1])
            assert np.concatenate([b1, b2]).tobytes() == whole["bases"][:nb].tobytes(), cut
            assert np.concatenate([q1, q2]).tobytes() == whole["quals"][:nb].tobytes(), cut
            assert np.array_equal(np.concatenate([o1[:-1], o2 + o1[-1]]), whole["offsets"]), cut
            r2 = r2.copy()
            for f in ("head_pos", "seq_pos", "qual_pos"):
                r2[f] += info["consumed"]
            assert np.concatenate([r1, r2]).tobytes() == whole["recs"].tobytes(), cut
            assert all(info[f] + info2[f] == whole["info"][f] for f in PR.SUMMED), cut
        # Parser.stream does the carry-over on a file
        for window in (3, 50, 64, 1000):
            want = PR.stream(text, PC.FASTQ, window, True)
            n = 0
            for info, (chunk, w) in zip(p.stream(io.BytesIO(text), window), want):
                check(p, g, info, w, ("stream", window, n))
                n += 1
            assert n == len(want)
        res["consumed_0_in_stream_of_3"] = PR.stream(text, PC.FASTQ, 3, True)[0][1]["info"]["consumed"]
    assert res["consumed_0"] >= 1
    return res


def device_input():
    """chunk_device on a 16-byte aligned sub-range of a larger buffer whose every other byte -- in front, behind, and between n_bytes
    and its round-up to 16 -- is a newline or a marker: the batch is the one of the text alone, and the buffer is not written"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(9)
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(PC.FASTQ, True) as p:
        for front, n_reads, cut in ((16, 40, 0), (4096 + 48, 300, 1), (160, 300, 7), (32, 1, 3)):
            text = PC.fastq(rng, rng.integers(0, 120, n_reads))
            text = text[:len(text) - cut]   # ends 0, 1, 7, 3 bytes early: every distance to the next 16-byte boundary matters
            size = front + len(text) + 80
            size += -size % 16
            host = np.frombuffer((b"\n@" * size)[:size], dtype=np.uint8).copy()
            host[front:front + len(text)] = np.frombuffer(text, dtype=np.uint8)
            d = g.malloc(size)
            try:
                d.from_host(host)
                for last in (True, False):
                    info = p.chunk_device(d.ptr + front, len(text), last)
                    check(p, g, info, PR.parse(text, PC.FASTQ, True, last), ("device", front, last))
                    if last:
                        res["front_%d" % front] = {"n_records": info["n_records"], "tail": len(text) % 16}
                assert np.array_equal(d.to_host(np.uint8, size), host), "the text was written"
            finally:
                d.free()
    assert {v["tail"] for v in res.values()} - {0} and len(res) == 4
    return res


def lowqual():
    """reads.fq and mixed.fq: the parsed batch, where it lies, through Cleaner.lowqual_device and compact() equals the same calls on
    host-built arrays, and the reference's golden output"""
    from dbg_assembly_amd import capi
    import clean_compact_restatement as CC
    import clean_restatement as CR
    res = {}
    with capi.Cleaner() as c, capi.Cleaner() as c_host, capi.Parser(PC.FASTQ, True) as p:
        for case in CR.golden_cases(PC.CLEAN):
            if case["program"] != "clean_lowqual" or case["input"].split(".")[0] not in ("reads", "mixed"):
                continue
            b = CC.golden_batch(PC.CLEAN, case)
            path = os.path.join(PC.CLEAN, case["input"])
            text = (gzip.open if path.endswith(".gz") else open)(path, "rb").read()
            info = p.chunk(text)
            d_b, d_q, _, n, nb = p.device()
            _, _, offsets, _ = p.results()
            rec = c.lowqual_device(d_b, d_q, offsets, b["opts"]["-e"], b["opts"]["-q"])
            cnt = c.compact(b["opts"]["-r"])
            bases, quals, off = c.compact_to_host()
            hb, hoff = CC.pack(b["reads"])
            hq, _ = CC.pack(b["quals"])
            assert np.array_equal(hoff, offsets), case["name"]
            rec_h = c_host.lowqual(hb, hq, hoff, b["opts"]["-e"], b["opts"]["-q"])
            cnt_h = c_host.compact(b["opts"]["-r"])
            bases_h, quals_h, off_h = c_host.compact_to_host()
            assert rec.tobytes() == rec_h.tobytes() and np.array_equal(bases, bases_h) and np.array_equal(quals, quals_h), case["name"]
            assert np.array_equal(off, off_h) and all(cnt[f] == cnt_h[f] for f in CC.COUNTERS), case["name"]
            assert CC.as_lines(bases, off) == b["lines2"] and CC.as_lines(quals, off) == b["lines4"], case["name"]
            assert {f: cnt[f] for f in CC.COUNTERS} == b["stat"], (case["name"], cnt, b["stat"])
            res[case["name"]] = {"input": case["input"], "reads": info["n_records"], "mismatched": info["mismatched"]}
    return res


def reads_150(n, seed):
    from oracle import oracle_py as O
    bases, offsets = O.synth_reads(O.synth_params(20000, 150, cfg=1), seed * 100000, n)
    raw = np.ascontiguousarray(bases, dtype=np.uint8).tobytes()
    return [raw[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def graph():
    """the parsed batch pushed into a k = 31 graph, DIRECT and PARTITION, against the same reads through push_reads; then a text in
    two chunks, the second one parsed while the first batch is still lent to the graph handle"""
    from dbg_assembly_amd import capi
    from clean_compact_gpu_steps import graph_args, result_of, same
    reads = reads_150(3000, 7)
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, PC.qual_of(i, len(r))) for i, r in enumerate(reads))
    whole = PR.parse(text, PC.FASTQ)
    assert [s for _, s, _ in whole["records"]] == reads
    nb = int(whole["offsets"][-1])
    res = {}
    with capi.Parser(PC.FASTQ) as p:
        for engine in ("direct", "partition"):
            with capi.Graph(**graph_args(capi, engine, 3000)) as g:
                g.push_reads(np.ascontiguousarray(whole["bases"][:nb]), whole["offsets"])
                old = result_of(g)
                digest_old = g.digest()
            with capi.Graph(**graph_args(capi, engine, 3000)) as g:
                info = p.chunk(text)
                assert info["n_records"] == 3000
                g.push_parsed(p)
                new = result_of(g)
                digest_new = g.digest()
            same(new, old, engine)
            assert digest_new == digest_old, engine
            with capi.Graph(**graph_args(capi, engine, 3000)) as g:   # no sync of the graph between the push and the next chunk
                cut = len(text) * 2 // 3
                first = p.chunk(text[:cut], last=False)
                g.push_parsed(p)
                second = p.chunk(text[first["consumed"]:], last=True)
                g.push_parsed(p)
                assert 0 < first["n_records"] < 3000 and first["n_records"] + second["n_records"] == 3000
                lent = result_of(g)
            same(lent, old, engine + " in two chunks")
            res[engine] = {"reads": new[0][0], "nodes": new[0][2]}
    return res


def status_of(call):
    from dbg_assembly_amd import capi
    try:
        call()
    except capi.DbgkError as e:
        return e.status
    return capi.OK


def states():
    from dbg_assembly_amd import capi
    res = {}
    h = ctypes.c_void_p()
    res["with_quals_for_fasta"] = capi.lib().dbgk_parse_create(2, 1, 0, ctypes.byref(h))
    res["format_3"] = capi.lib().dbgk_parse_create(3, 0, 0, ctypes.byref(h))
    text = b"@r\nACGT\n+\nIIII\n"
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(PC.FASTQ, True) as p, capi.Parser(PC.FASTQ) as bare:
        res["results_before_a_chunk"] = status_of(p.results)
        res["device_before_a_chunk"] = status_of(p.device)
        res["push_before_a_chunk"] = status_of(lambda: g.push_parsed(p))
        res["n_bytes_2_to_the_31"] = capi.lib().dbgk_parse_chunk(p._h, text, 1 << 31, 1, ctypes.byref(capi.ParseInfo()))
        d = g.malloc(64)
        d.from_host(np.frombuffer(text.ljust(64, b"\n"), dtype=np.uint8))
        res["n_bytes_2_to_the_31_device"] = status_of(lambda: p.chunk_device(d.ptr, 1 << 31))
        res["misaligned_text"] = status_of(lambda: p.chunk_device(d.ptr + 4, 8))
        res["results_after_a_refused_chunk"] = status_of(p.results)
        res["empty_chunk"] = status_of(lambda: p.chunk(b""))
        res["empty_chunk_device"] = status_of(lambda: p.chunk_device(None, 0))
        info = p.chunk_device(d.ptr, len(text))
        assert info["n_records"] == 1 and info["n_bases"] == 4
        d_b, d_q, _, _, _ = p.device()
        res["own_bases_as_input"] = status_of(lambda: p.chunk_device(d_b, 4))
        res["own_quals_as_input"] = status_of(lambda: p.chunk_device(d_q, 4))
        res["results_after_refused_input"] = status_of(p.results)
        bare.chunk(text)
        q = np.zeros(16, dtype=np.uint8)
        res["quality_plane_of_a_batch_without_one"] = capi.lib().dbgk_parse_results(bare._h, None, q.ctypes.data, None, None)
        res["results_with_no_pointer"] = capi.lib().dbgk_parse_results(bare._h, None, None, None, None)
        d.free()
        g.finalize()
        res["push_into_a_finalized_handle"] = status_of(lambda: g.push_parsed(p))
    return res


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "many": many, "chunking": chunking, "device_input": device_input, "lowqual": lowqual, "graph": graph,
                      "states": states}[sys.argv[1]]()))
