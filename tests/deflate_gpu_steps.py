"""GPU steps of tests/test_deflate_gpu.py, each run in a child process of its own under a time limit:
    python tests/deflate_gpu_steps.py crafted | rounds | repeat | device_input | streaming | handover | states
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
import deflate_cases as DC  # noqa: E402
import deflate_restatement as DR  # noqa: E402


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], dtype=np.uint8) != np.frombuffer(b[:n], dtype=np.uint8))
    return (len(a), len(b), int(d[0]) if d.size else n)


def crafted():
    """every crafted case at every level through Deflater.deflate: the restatement's bytes, gzip's verdict, the counters"""
    from dbg_assembly_amd import capi
    res = {}
    for level in DC.LEVELS:
        with capi.Deflater(level) as z:
            for name, data in DC.cases().items():
                want, info = DR.deflate(data, level)
                got = z.deflate(data)
                assert got == want, (name, level, first_difference(got, want))
                assert gzip.decompress(got) == data, (name, level)
                assert z.info == info, (name, level, z.info, info)
                if level == DR.MAX_LEVEL:
                    res[name] = {f: info[f] for f in ("n_members", "out_bytes", "stored_members", "n_matches")}
            t = z.timing()
            phases = [t[f] for f in ("ms_match", "ms_crc_hist", "ms_codes", "ms_encode")]
            assert t["ms_members"] > 0 and t["ms_compact"] > 0 and abs(sum(phases) - t["ms_members"]) <= 1e-9 * t["ms_members"]
            assert (t["ms_match"] > 0) == (level == 2) and t["ms_crc_hist"] > 0 and t["ms_encode"] > 0 and (t["ms_codes"] > 0) == (level > 0)
    return res


def rounds():
    """more members than the member kernel's grid holds: workgroups take a second piece, a poorer one, behind their first"""
    from dbg_assembly_amd import capi
    text, n = DC.rounds_text()
    memo = {}
    out, stored = [], 0
    for i in range(0, len(text), DR.PIECE):
        piece = text[i:i + DR.PIECE]
        if piece not in memo:
            memo[piece] = DR.member(piece, DR.MAX_LEVEL)
        out.append(memo[piece][0])
        stored += memo[piece][1]
    want = b"".join(out) + DR.MARKER
    with capi.Deflater() as z:
        got = z.deflate(text)
        assert got == want, first_difference(got, want)
        assert z.info["n_members"] == n and z.info["stored_members"] == stored and z.info["out_bytes"] == len(want)
        res = dict(z.info, distinct_pieces=len(memo), **z.timing())
    assert len(DR.walk(got)) == n + 1
    return res


def repeat():
    """the same input twice through one handle and once through a second one; a smaller input in between leaves nothing behind"""
    from dbg_assembly_amd import capi
    text = DC.fastq_like(3 * DR.PIECE + 77, seed=8)
    res = {}
    for level in DC.LEVELS:
        with capi.Deflater(level) as a, capi.Deflater(level) as b:
            first = a.deflate(text)
            small = a.deflate(text[:1000])
            second = a.deflate(text)
            other = b.deflate(text)
            assert first == second == other and gzip.decompress(first) == text and gzip.decompress(small) == text[:1000], level
            assert a.results() == second
        res["level_%d" % level] = len(first)
    return res


def device_input():
    """deflate_device on a 16-byte aligned sub-range of a larger buffer of other bytes gives the bytes of the host call, and the
    buffer is not written"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(4)
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Deflater() as z, capi.Deflater() as z_host:
        for front, n in ((16, 1), (48, 5000), (4096 + 32, DR.PIECE), (160, DR.PIECE + 3), (32, 2 * DR.PIECE - 9)):
            text = DC.fastq_like(n, seed=front)
            size = front + n + 80
            size += -size % 16
            host = rng.integers(0, 256, size, dtype=np.uint8)
            host[front:front + n] = np.frombuffer(text, dtype=np.uint8)
            d = g.malloc(size)
            try:
                d.from_host(host)
                for last in (True, False):
                    got = z.deflate_device(d.ptr + front, n, last)
                    want = z_host.deflate(text, last)
                    assert got == want == DR.deflate(text, DR.MAX_LEVEL, last)[0], (front, last)
                    assert z.info == z_host.info
                ptr, n_out = z.device()
                assert n_out == len(got) and ptr % 16 == 0
                assert np.array_equal(d.to_host(np.uint8, size), host), "the text was written"
                res["front_%d" % front] = {"tail": n % 16, "out": n_out}
            finally:
                d.free()
    assert {v["tail"] for v in res.values()} - {0} and len(res) == 5
    return res


def streaming():
    """a small text through stream() with windows of every size from 1 to its length and beyond: the members of all windows inflate
    to the text, and the end marker stands once, at the end"""
    from dbg_assembly_amd import capi
    text = DC.fastq_like(150, seed=3)
    res = {"windows": 0}
    with capi.Deflater() as z:
        for window in list(range(1, len(text) + 2)) + [1000]:
            dst = io.BytesIO()
            total = z.stream(io.BytesIO(text), dst, window)
            out = dst.getvalue()
            n = -(-len(text) // window)
            assert gzip.decompress(out) == text, window
            ms = DR.walk(out)
            assert len(ms) == n + 1 and [m[2] for m in ms] == [min(window, len(text) - i * window) for i in range(n)] + [0], window
            assert out.endswith(DR.MARKER) and out.count(DR.MARKER) == 1 and total["n_members"] == n and total["out_bytes"] == len(out), window
            want = b"".join(DR.deflate(text[i:i + window], DR.MAX_LEVEL, last=i + window >= len(text))[0] for i in range(0, len(text), window))
            assert out == want, window
            res["windows"] += 1
        dst = io.BytesIO()
        z.stream(io.BytesIO(b""), dst, 64)
        assert dst.getvalue() == DR.MARKER
        # larger windows that are no multiple of a piece: a short member ends every window
        big = DC.fastq_like(3 * DR.PIECE, seed=6)
        dst = io.BytesIO()
        z.stream(io.BytesIO(big), dst, DR.PIECE + 100)
        assert gzip.decompress(dst.getvalue()) == big and [m[2] for m in DR.walk(dst.getvalue())] == [DR.PIECE, 100, DR.PIECE, 100, DR.PIECE - 200, 0]
    return res


def handover():
    """a PARSE golden text, uploaded once: parsed where it lies, deflated where it lies; the members, inflated on the host and
    parsed again, give the same batch"""
    from dbg_assembly_amd import capi
    import parse_cases as PC
    path = os.path.join(PC.CLEAN, "reads.fq")
    text = open(path, "rb").read()
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Parser(PC.FASTQ, True) as p, capi.Deflater() as z:
        size = len(text) + 64
        size += -size % 16
        d = g.malloc(size)
        try:
            d.from_host(np.frombuffer(text.ljust(size, b"\n"), dtype=np.uint8))
            info = p.chunk_device(d.ptr, len(text))
            first = [a.copy() if a is not None else None for a in p.results()]
            packed = z.deflate_device(d.ptr, len(text))
        finally:
            d.free()
        assert packed == DR.deflate(text, DR.MAX_LEVEL)[0]
        inflated = gzip.decompress(packed)
        assert inflated == text
        info2 = p.chunk(inflated)
        second = p.results()
        assert all(info[f] == info2[f] for f in ("n_records", "n_lines", "n_bases", "mismatched", "max_len", "consumed"))
        assert all(np.array_equal(a, b) for a, b in zip(first, second)) and info["n_records"] > 0
        res = {"records": info["n_records"], "text": len(text), "packed": len(packed)}
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
    L = capi.lib()
    res = {}
    h = ctypes.c_void_p()
    res["level_3"] = L.dbgk_gz_create(3, ctypes.byref(h))
    res["level_above_the_built_ones"] = L.dbgk_gz_create(capi.GZ_MAX_LEVEL + 1, ctypes.byref(h))
    res["level_minus_1"] = L.dbgk_gz_create(-1, ctypes.byref(h))
    text = b"@r\nACGT\n+\nIIII\n"
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Deflater() as z:
        res["results_before_a_call"] = status_of(z.results)
        res["device_before_a_call"] = status_of(z.device)
        res["n_bytes_2_to_the_31"] = L.dbgk_gz_deflate(z._h, text, 1 << 31, 1, ctypes.byref(capi.GzInfo()))
        d = g.malloc(64)
        d.from_host(np.frombuffer(text.ljust(64, b"\n"), dtype=np.uint8))
        res["n_bytes_2_to_the_31_device"] = status_of(lambda: z.deflate_device(d.ptr, 1 << 31))
        res["misaligned_text"] = status_of(lambda: z.deflate_device(d.ptr + 4, 8))
        res["results_after_a_refused_call"] = status_of(z.results)
        res["empty_without_last"] = status_of(lambda: z.deflate(b"", last=False))
        assert z.results() == b"" and z.device() == (None, 0) and z.info["n_members"] == 0
        res["empty_device_with_last"] = status_of(lambda: z.deflate_device(None, 0))
        assert z.results() == DR.MARKER
        got = z.deflate_device(d.ptr, len(text))
        assert gzip.decompress(got) == text
        ptr, n = z.device()
        res["own_output_as_input"] = status_of(lambda: z.deflate_device(ptr, 16))
        res["results_after_refused_input"] = status_of(z.results)
        out = np.zeros(n, dtype=np.uint8)
        res["capacity_one_short"] = L.dbgk_gz_results(z._h, out.ctypes.data, n - 1)
        res["capacity_exact"] = L.dbgk_gz_results(z._h, out.ctypes.data, n)
        assert out.tobytes() == got
        res["null_info"] = L.dbgk_gz_deflate(z._h, text, len(text), 1, None)
        d.free()
    return res


def run_both(cmd, make_dir, cwd_of=None):
    """one command line in two fresh directories, without and with DBGK_GZ=device -> ({file: bytes} of both, relative names)"""
    import subprocess
    import tempfile
    outs = []
    for form in (None, "device"):
        with tempfile.TemporaryDirectory() as tmp:
            make_dir(tmp)
            env = {k: v for k, v in os.environ.items() if k != "DBGK_GZ"}
            if form:
                env["DBGK_GZ"] = form
            r = subprocess.run([a.replace("TMP", tmp) for a in cmd], env=env, capture_output=True, text=True, timeout=120,
                               cwd=cwd_of(tmp) if cwd_of else None)
            assert r.returncode == 0, (cmd, form, r.stderr[-2000:])
            files = {}
            for base, _, names in os.walk(tmp):
                for f in names:
                    p = os.path.join(base, f)
                    files[os.path.relpath(p, tmp)] = open(p, "rb").read().replace(tmp.encode(), b"TMP")
            outs.append(files)
    return outs


def compare_forms(plain, device, inputs):
    """every file but a .gz output byte-identical; every .gz output: the same bytes after inflation, zlib's header without the
    variable, BGZF members with one end marker with it -> {output: [plain bytes, device bytes, members]}"""
    assert sorted(plain) == sorted(device)
    res = {}
    for f in sorted(plain):
        if f in inputs or not f.endswith(".gz"):
            assert plain[f] == device[f], f
            continue
        assert plain[f][:4] == b"\x1f\x8b\x08\x00" and device[f][:4] == b"\x1f\x8b\x08\x04", f
        assert gzip.decompress(plain[f]) == gzip.decompress(device[f]), f
        ms = DR.walk(device[f])
        assert device[f].endswith(DR.MARKER) and [m[2] for m in ms].count(0) == 1 and sum(m[2] for m in ms) == len(gzip.decompress(plain[f])), f
        res[f] = [len(plain[f]), len(device[f]), len(ms)]
    return res


def programs():
    """bin/clean_lowqual, clean_adapter, correct_error_reads (with and without -j 1) and map_reads on one golden case each, without
    and with DBGK_GZ=device: the .gz outputs inflate to the same bytes -- the golden's --, every other file is byte-identical"""
    import shutil
    import clean_restatement as CR
    import map_restatement as MR
    import pair_gpu_steps as PG
    import pair_restatement as PR
    import test_clean_cpu as TC
    import test_correct_cpu as TO
    import test_map_cpu as TM
    res = {}
    # ---- the two cleaners
    for program in ("clean_lowqual", "clean_adapter"):
        case = next(c for c in TC.golden_cases() if c["program"] == program and c["input"] == "reads.fq")
        cmd = [os.path.join(TC.BIN, program)] + case["args"] + [case["input"], "TMP/out.gz", "TMP/out.stat"]
        plain, device = run_both(cmd, lambda tmp: None, cwd_of=lambda tmp: TC.CASES)
        res[program] = compare_forms(plain, device, ())
        want = CR.expected_outputs(TC.CASES, case)
        assert gzip.decompress(device["out.gz"]).decode("latin-1") == want["out"] and device["out.stat"].decode("latin-1") == want["stat"], program
        assert list(res[program]) == ["out.gz"]
    # ---- the corrector, one file
    d, case = TO.golden_cases()[0]
    D = os.path.join(TO.GOLDEN, d)

    def one_file(tmp):
        shutil.copy(os.path.join(D, case["reads"]), os.path.join(tmp, case["reads"]))
        open(os.path.join(tmp, "reads.lib"), "w").write("%s\n" % os.path.join(tmp, case["reads"]))
    plain, device = run_both([TO.EXE] + case["args"] + [os.path.join(D, "table.cz"), "TMP/reads.lib"], one_file)
    res["correct_error_reads"] = compare_forms(plain, device, (case["reads"],))
    assert gzip.decompress(device[case["reads"] + ".correct.fa.gz"]) == TO.expected_fa(d, case)
    assert device[case["reads"] + ".correct.stat"] == open(os.path.join(D, case["name"] + ".correct.stat"), "rb").read()
    assert list(res["correct_error_reads"]) == [case["reads"] + ".correct.fa.gz"]
    # ---- the corrector with -j 1: five .gz outputs
    name, (pcase, _, _) = next(iter(PR.CASES.items()))
    meta = {c["name"]: c for c in json.load(open(os.path.join(PR.CORRECT, "cases.json")))}

    def two_files(tmp):
        f1, f2 = os.path.join(tmp, "reads_1.fq.gz"), os.path.join(tmp, "reads_2.fq")
        shutil.copy(os.path.join(PR.CORRECT, "reads.fq.gz"), f1)
        PG.rotated_fq(f1, f2)
        open(os.path.join(tmp, "reads.lib"), "w").write("%s\n%s\n" % (f1, f2))
    plain, device = run_both([TO.EXE] + meta[pcase]["args"] + ["-j", "1", os.path.join(PR.CORRECT, "table.cz"), "TMP/reads.lib"], two_files)
    res["correct_error_reads_j1"] = compare_forms(plain, device, ("reads_1.fq.gz",))
    pair, single, stat = PG.golden(name)
    assert gzip.decompress(device["reads_1.fq.gz.correct.fa.gz.pair.fa.gz"]) == pair
    assert gzip.decompress(device["reads_1.fq.gz.correct.fa.gz.single.fa.gz"]) == single and device["reads_1.fq.gz.correct.fa.gz.pair.single.stat"] == stat
    assert len(res["correct_error_reads_j1"]) == 4
    # ---- the mapper
    case = next(c for c in TM.golden_cases() if c["program"] == "map_reads")

    def map_dir(tmp):
        os.mkdir(os.path.join(tmp, "in"))
        for f in os.listdir(TM.CASES):
            if os.path.isfile(os.path.join(TM.CASES, f)):
                shutil.copy(os.path.join(TM.CASES, f), os.path.join(tmp, "in", f))
    plain, device = run_both([os.path.join(TM.BIN, "map_reads")] + case["args"] + ["-o", "TMP/out", case["contigs"], case["lib"]], map_dir,
                             cwd_of=lambda tmp: os.path.join(tmp, "in"))
    inputs = tuple(os.path.join("in", f) for f in os.listdir(TM.CASES))
    res["map_reads"] = compare_forms(plain, device, inputs)
    want = MR.expected_outputs(TM.CASES, case)
    for f, text in want.items():
        if f.endswith(".gz"):
            assert gzip.decompress(device[os.path.join("out", f)]).decode("latin-1") == text, f
    for suffix in (".map_reads.2ctg.gz", ".map_reads.2ctg.gz.reads.fa.gz", ".map_reads.1ctg.gz"):   # (per read file of the library)
        assert any(f.endswith(suffix) for f in res["map_reads"]), suffix
    assert len(res["map_reads"]) == sum(1 for f in want if f.endswith(".gz"))
    return res


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "rounds": rounds, "repeat": repeat, "device_input": device_input, "streaming": streaming,
                      "handover": handover, "states": states, "programs": programs}[sys.argv[1]]()))
