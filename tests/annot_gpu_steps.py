"""GPU steps of tests/test_annot_gpu.py, each run in a child process of its own under a time limit:
    python tests/annot_gpu_steps.py crafted | formatter | states | chain
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
import annot_cases as AC  # noqa: E402
import annot_restatement as AR  # noqa: E402
import format_cases as FC  # noqa: E402
import format_restatement as FR  # noqa: E402
from format_gpu_steps import check as check_text, formatters, place  # noqa: E402
from parse_gpu_steps import fetch, status_of  # noqa: E402


def check_plane(c, g, got, want, name):
    """annotate() and the plane where it lies against the restatement: the bytes, the offsets, and the whole 16-byte vectors on the
    device with the zero pad"""
    plane, off = want
    suffix, offsets = got
    assert np.array_equal(offsets, off), (name, "offsets")
    assert np.array_equal(suffix, plane), (name, int(np.flatnonzero(suffix != plane)[0]) if suffix.size == plane.size else (suffix.size, plane.size))
    info = c.annot_info
    assert (info["n"], info["suffix_bytes"]) == (len(off) - 1, plane.size), (name, info)
    dev = c.annotate_device()
    assert (dev.n, dev.n_bytes) == (len(off) - 1, plane.size) and dev.d_suffix and dev.d_suffix % 16 == 0 and dev.d_offsets % 8 == 0, name
    vec, image = fetch(g, dev.d_suffix, -(-plane.size // 16) * 16), AR.vectors(plane)
    assert np.array_equal(vec, image), (name, int(np.flatnonzero(vec != image)[0]))
    assert np.array_equal(fetch(g, dev.d_offsets, 8 * len(off)).view(np.uint64), off), (name, "offsets on the device")
    if not plane.size:
        assert info["ms_write"] == 0
    return {"n": info["n"], "suffix_bytes": info["suffix_bytes"]}


def crafted():
    """every crafted batch through compact_from + annotate on ONE handle, in the order of the cases (a small batch after a large one
    is the last pair)"""
    from dbg_assembly_amd import capi
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Corrector(k=5) as c:
        for name, case in AC.cases().items():
            bases, offsets = AC.batch(case)
            c.compact_from(bases, offsets, case["rec"])
            _, coff = c.compact_to_host()
            assert np.array_equal(np.diff(coff.astype(np.int64)), AC.compact_lengths(case).astype(np.int64)), name
            res[name] = check_plane(c, g, c.annotate(), AC.expected(case), name)
    return res


def suffix_cases():
    return {name: c for name, c in FC.cases().items() if c["suffixes"] is not None and any(c["suffixes"])}


def upload_suffixes(g, capi, suffixes, front=32):
    """the suffixes as a plane inside larger device buffers of other bytes -> (DeviceSuffixes, buffers)"""
    off = np.zeros(len(suffixes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in suffixes])
    d_s, _ = place(g, b"".join(suffixes), front, b"\n>\t")
    d_o, _ = place(g, off.view(np.uint8), 16, b"\xff")
    return capi.DeviceSuffixes(d_s.ptr + front, d_o.ptr + 16, len(suffixes), int(off[-1])), [d_s, d_o]


def formatter():
    """the crafted cases of tests/format_cases.py that have suffixes: the text and the counters with the plane on the device are those
    of the host-suffix call, which are the restatement's"""
    from dbg_assembly_amd import capi
    res = {}
    made, get = formatters(capi)
    cases = suffix_cases()
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        try:
            for name, c in cases.items():
                f = get(c["fmt"], c["marker"])
                n = len(c["recs"])
                bufs = [place(g, c["text"], 16, b"\n@>")[0], place(g, c["recs"].view(np.uint8), 16, b"\x07")[0], place(g, c["bases"], 16, b"\nA>")[0],
                        place(g, c["offsets"].view(np.uint8), 32, b"\xff")[0]]
                if c["quals"] is not None:
                    bufs.append(place(g, c["quals"], 16, b"\nI@")[0])
                dev, sbufs = upload_suffixes(g, capi, c["suffixes"])
                try:
                    source = (bufs[0].ptr + 16, len(c["text"]), bufs[1].ptr + 16)
                    planes = (bufs[2].ptr + 16, bufs[4].ptr + 16 if c["quals"] is not None else None, bufs[3].ptr + 32, n)
                    host_info = f.format_device(source, planes, c["suffixes"])
                    host_text = f.results()
                    info = f.format_device(source, planes, dev)
                    res[name] = check_text(f, g, info, FC.expected(c), name)
                    assert f.results() == host_text and {k: info[k] for k in FR.COUNTERS} == {k: host_info[k] for k in FR.COUNTERS}, name
                finally:
                    for d in bufs + sbufs:
                        d.free()
        finally:
            for f in made.values():
                f.close()
    return res


def states():
    from dbg_assembly_amd import capi
    L = capi.lib()
    res = {}
    c = FC.build(FC.FASTA, [b">a", b">bc"], [b"ACGT", b"AC"], suffixes=[b"\tx", b"\tyz"], marker=0)
    n = 2
    p, u = ctypes.c_void_p(), ctypes.c_uint64()
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Formatter(FC.FASTA) as fa, capi.Corrector(k=5) as corr:
        # the corrector's side
        info = capi.CorrAnnotInfo()
        res["annot_before_a_compact_batch"] = L.dbgk_corr_annot(corr._h, ctypes.byref(info))
        res["annot_device_before_a_compact_batch"] = L.dbgk_corr_annot_device(corr._h, ctypes.byref(p), ctypes.byref(p), ctypes.byref(u), ctypes.byref(u))
        case = AC.cases()["deleted"]
        bases, offsets = AC.batch(case)
        corr.compact_from(bases, offsets, case["rec"])
        res["annot_device_before_annot"] = L.dbgk_corr_annot_device(corr._h, ctypes.byref(p), ctypes.byref(p), ctypes.byref(u), ctypes.byref(u))
        res["annot_results_before_annot"] = L.dbgk_corr_annot_results(corr._h, None, None)
        res["annot"] = status_of(corr.annotate)
        res["annot_device_after_annot"] = L.dbgk_corr_annot_device(corr._h, ctypes.byref(p), ctypes.byref(p), ctypes.byref(u), ctypes.byref(u))
        corr.compact_from(bases, offsets, case["rec"])
        res["annot_device_after_the_next_compact"] = L.dbgk_corr_annot_device(corr._h, ctypes.byref(p), ctypes.byref(p), ctypes.byref(u), ctypes.byref(u))
        # the formatter's side
        bufs = {k: place(g, v, 16, b"\n")[0] for k, v in (("text", c["text"]), ("recs", c["recs"].view(np.uint8)), ("bases", c["bases"]),
                                                           ("off", c["offsets"].view(np.uint8)), ("suf", b"\tx\tyz"))}
        at = {k: d.ptr + 16 for k, d in bufs.items()}

        def soff(*v):
            d = place(g, np.array(v, dtype=np.uint64).view(np.uint8), 16, b"\n")[0]
            bufs["soff%d" % len(bufs)] = d
            return d.ptr + 16

        def dev(d_suffix, d_soff):
            return status_of(lambda: fa.format_device((at["text"], len(c["text"]), at["recs"]), (at["bases"], None, at["off"], n),
                                                      capi.DeviceSuffixes(d_suffix, d_soff, n, 0)))
        good = soff(0, 2, 5)
        res["results_before_a_call"] = status_of(fa.results)
        res["good_call"] = dev(at["suf"], good)
        assert fa.results() == FC.expected(c)[0]
        res["offsets_from_1"] = dev(at["suf"], soff(1, 2, 5))
        res["results_after_offsets_from_1"] = status_of(fa.results)
        res["good_call_again"] = dev(at["suf"], good)
        res["decreasing_offsets"] = dev(at["suf"], soff(0, 3, 2))
        res["results_after_decreasing_offsets"] = status_of(fa.results)
        res["total_of_2_to_the_32"] = dev(at["suf"], soff(0, 2, 1 << 32))
        res["results_after_a_total_of_2_to_the_32"] = status_of(fa.results)
        res["total_of_2_to_the_32_less_1_without_a_plane"] = dev(None, soff(0, 2, (1 << 32) - 1))
        res["good_call_once_more"] = dev(at["suf"], good)
        assert fa.results() == FC.expected(c)[0]
        res["misaligned_plane"] = dev(at["suf"] + 4, good)
        res["misaligned_offsets"] = dev(at["suf"], good + 4)
        d_out, _ = fa.device()
        res["own_output_as_plane"] = dev(d_out, good)
        res["results_after_refused_arguments"] = status_of(fa.results)
        res["no_plane_at_all"] = dev(None, None)
        assert fa.results() == FR.format_batch(FC.FASTA, c["text"], c["recs"], c["bases"], None, c["offsets"], None, 0)[0]
        res["all_empty_suffixes"] = dev(None, soff(0, 0, 0))
        for d in bufs.values():
            d.free()
    return res


def golden_batches():
    """every correct_* golden case and every pinned edge scenario with a committed table: (name, corrector options, table file,
    format, text of the input file, the reference's .correct.fa)"""
    import correct_edge_cases as E
    from test_correct_cpu import GOLDEN, expected_fa, golden_cases, params_of
    out = []
    for d, case in golden_cases():
        P = params_of(case)
        text = gzip.open(os.path.join(GOLDEN, d, case["reads"]), "rb").read() if case["reads"].endswith(".gz") else open(os.path.join(GOLDEN, d, case["reads"]), "rb").read()
        out.append(("%s/%s" % (d, case["name"]), dict(k=P.k, m=P.m, c=P.c, x=P.x, n=P.n, r=P.r), os.path.join(GOLDEN, d, "table.cz"), case["format"], text,
                    expected_fa(d, case)))
    edges = os.path.join(GOLDEN, "correct_edges")
    for meta in json.load(open(os.path.join(edges, "cases.json"))):
        if not meta["table"]:
            continue
        s = E.scenario(meta["name"])
        out.append(("correct_edges/" + meta["name"], dict(k=s.k, **s.opts), os.path.join(edges, meta["table"]), 2,
                    gzip.open(os.path.join(edges, meta["reads"]), "rb").read(), gzip.open(os.path.join(edges, meta["name"] + ".correct.fa.gz"), "rb").read()))
    return out


def chain():
    """Parser -> Corrector.correct_device -> compact -> annotate_device -> Formatter where everything lies: the text is the file the
    reference wrote; parsed again where it lies it is the compact batch under the annotated headers; deflated where it lies and
    inflated by zlib it is the same text"""
    from dbg_assembly_amd import capi
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(FC.FASTA) as p2, capi.Formatter(FC.FASTA, b">") as f, \
            capi.Deflater() as z:
        for name, opts, table, fmt, text, want in golden_batches():
            with capi.Corrector(**opts) as c, capi.Parser(fmt) as p:
                c.load_file(table)
                p.chunk(text)
                d_b, _, _, n, _ = p.device()
                _, _, offsets, recs = p.results()
                rec = c.correct_device(d_b, offsets)
                c.compact()
                dev = c.annotate_device()
                fi = f.format_device(p, c.compact_device()[:1] + (None,) + c.compact_device()[1:3], dev)
                got = f.results()
                assert got == want, (name, "the text differs from the reference's file")
                cb, coff = c.compact_to_host()
                plane, soff = AR.suffixes(rec, np.diff(coff.astype(np.int64)))
                sufs = AR.split(plane, soff)
                check_text(f, g, fi, FR.format_batch(FC.FASTA, text, recs, cb, None, coff, sufs, ord(">")), name)
                d_out, n_out = f.device()
                back = p2.chunk_device(d_out, n_out)
                b2, _, o2, r2 = p2.results()
                assert back["n_records"] == n and back["ignored_lines"] == 0, name
                assert np.array_equal(o2, coff) and np.array_equal(b2, cb), name
                heads = [b">" + text[int(r["head_pos"]) + 1:int(r["head_pos"]) + int(r["head_len"])] for r in recs]
                assert [got[int(r["head_pos"]):int(r["head_pos"]) + int(r["head_len"])] for r in r2] == [h + s for h, s in zip(heads, sufs)], name
                assert gzip.decompress(z.deflate_device(d_out, n_out)) == want, name
                res[name] = {"records": n, "suffix_bytes": fi["suffix_bytes"], "out_bytes": fi["out_bytes"]}
    return res


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "formatter": formatter, "states": states, "chain": chain}[sys.argv[1]]()))
