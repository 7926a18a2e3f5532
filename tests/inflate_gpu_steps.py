"""GPU steps of tests/test_inflate_gpu.py, each run in a child process of its own under a time limit:
    python tests/inflate_gpu_steps.py crafted | corrupt | rounds | repeat | streaming | max_out | device_input | roundtrip | states | programs
Prints one JSON line of findings; exits non-zero on a mismatch.  zlib is the arbiter of bytes and verdicts everywhere."""
import ctypes
import gzip
import io
import json
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_cases as DC  # noqa: E402
import deflate_restatement as DR  # noqa: E402
import inflate_cases as IC  # noqa: E402

COUNTERS = ("n_stored", "n_fixed", "n_dynamic", "n_literals", "n_matches")


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], dtype=np.uint8) != np.frombuffer(b[:n], dtype=np.uint8))
    return (len(a), len(b), int(d[0]) if d.size else n)


def status_of(call):
    from dbg_assembly_amd import capi
    try:
        call()
    except capi.DbgkError as e:
        return e.status
    return capi.OK


def poke(g, ptr, data):
    from dbg_assembly_amd import capi
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8))
    capi._chk(capi.lib().dbgk_memcpy_h2d(g._h, ptr, a.ctypes.data, a.size), "dbgk_memcpy_h2d")


def peek(g, ptr, n):
    from dbg_assembly_amd import capi
    out = np.empty(n, dtype=np.uint8)
    capi._chk(capi.lib().dbgk_memcpy_d2h(g._h, out.ctypes.data, ptr, n), "dbgk_memcpy_d2h")
    return out.tobytes()


def crafted():
    """every valid case, a group per call: zlib's bytes, no member refused, the frame counters, and the block and token counters that
    tests/deflate_tokens.py lists for the group's members (the lister takes about a minute over all of them)"""
    from dbg_assembly_amd import capi
    res = {}
    with capi.Inflater() as z:
        for group, cases in IC.valid_groups().items():
            data = b"".join(m for _, m, _ in cases)
            want = b"".join(t for _, _, t in cases)
            assert gzip.decompress(data) == want, group
            got, info = z.inflate(data)
            assert got == want, (group, first_difference(got, want))
            ms = IC.split(data)
            assert (info["n_members"], info["n_markers"], info["consumed"], info["out_bytes"], info["n_bad"]) == \
                (len(ms), sum(m == DR.MARKER for m in ms), len(data), len(want), 0), (group, info)
            assert not z.member_status().any()
            assert {f: info[f] for f in COUNTERS} == IC.counters(data), (group, info)
            t = z.timing()
            assert t["ms_decode"] > 0 and t["ms_resolve"] > 0 and t["ms_scan"] > 0
            res[group] = dict(info, cases=len(cases), **t)
    return res


def corrupt():
    """Run only after the CPU sanitizer test of this stage (tests/test_inflate_cpu.py) has passed on the same tree: it sends the same
    corrupt members through the same decode core, and what the sanitizers did not find on the host is what may be sent to a device.
    One call whose members alternate good and corrupt: verdicts and reasons per member, every good member's bytes exact, every bad
    member's range zero, the 64 bytes behind the output untouched."""
    from dbg_assembly_amd import capi
    good = [(n, m, t) for n, ms, t in IC.valid_groups(own=False)["small"] for m in IC.split(ms) for t in [IC.verdict(m)]]
    bad = [(n, m, r) for n, m, r, device_only in IC.corrupt_cases() if not device_only]
    members, want, reasons = [], [], []
    for i, (name, m, r) in enumerate(bad):
        _, gm, gt = good[i % len(good)]
        members += [gm, m]
        isize = struct.unpack_from("<I", m, len(m) - 4)[0]
        want += [gt, bytes(isize)]
        reasons += [0, r]
        assert IC.verdict(m) is None and IC.verdict(gm) == gt
    data, want = b"".join(members), b"".join(want)
    pattern = bytes(range(37, 101))
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Inflater() as z:
        z.inflate(good[0][1])                      # the output buffer exists from here on: 1 MiB at the least
        ptr, _ = z.device_ptr()
        assert len(want) + 64 < (1 << 20)
        poke(g, ptr + len(want), pattern)
        got, info = z.inflate(data)
        assert z.device_ptr() == (ptr, len(want))
        status = z.member_status().tolist()
        assert status == reasons, [(i, IC.REASONS[a], IC.REASONS[b]) for i, (a, b) in enumerate(zip(status, reasons)) if a != b]
        assert got == want, first_difference(got, want)
        assert peek(g, ptr + len(want), 64) == pattern, "bytes behind the output were written"
        assert (info["n_bad"], info["first_bad"], info["first_bad_reason"]) == (len(bad), 1, reasons[1])
    return {"members": len(members), "bad": len(bad), "reasons": sorted(set(reasons))}


def dynamic_members():
    """-> f(text): a member of dynamic blocks of 40 literals each, written by hand (zlib codes so short a text with fixed codes):
    254 literal codes of 8 bits, 254, 255, end-of-block and one length symbol of 9, no distance code"""
    lens = [8] * 254 + [9] * 4
    head = IC.dynamic(IC.W(), lens, [0], [], final=0, eob=False)
    rest_v, rest_n = head.v >> 1, head.n - 1          # the block header behind its BFINAL bit
    rev = {sym: (int(format(c, "0%db" % n)[::-1], 2), n) for sym, (c, n) in IC.codes_of(lens).items()}

    def member(text):
        w = IC.W()
        for a in range(0, len(text), 40):
            w.put(1 if a + 40 >= len(text) else 0, 1).put(rest_v, rest_n)
            for b in text[a:a + 40]:
                w.put(*rev[b])
            w.put(*rev[256])
        return IC.frame(w.bytes(), text)
    return member


def rounds():
    """more members than one round of the token area and than any grid: 20 000 short ones of three kinds in rotation -- stored, fixed,
    dynamic in several blocks -- and a few full ones, the third of them with hundreds of blocks"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(5)
    text = DC.fastq_like(4000, seed=23)
    members, want = [], []
    dynamic = dynamic_members()
    kinds = (lambda t: IC.zmember(t, 0), lambda t: IC.zmember(t, 6, 8, zlib.Z_FIXED), dynamic)
    blocks = [0, 0, 0]
    for i in range(20000):
        n, at = int(rng.integers(1, 201)), int(rng.integers(0, 3800))
        members.append(kinds[i % 3](text[at:at + n]))
        want.append(text[at:at + n])
        blocks[i % 3] += -(-n // 40) if i % 3 == 2 else 1
        if i % 5000 == 2500:
            full = DC.fastq_like(DR.PIECE, seed=i)
            members.append(IC.zmember(full, (0, 6, 6, 6)[i // 5000], (8, 8, 1, 1)[i // 5000], (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, 0, 0)[i // 5000]))
            want.append(full)
    assert all(IC.verdict(m) == t for m, t in zip(members[:3000], want))
    data, want = b"".join(members), b"".join(want)
    assert len(members) > 5 * capi.INF_ROUND
    with capi.Inflater() as z:
        got, info = z.inflate(data)
        assert got == want, first_difference(got, want)
        assert info["n_bad"] == 0 and info["n_members"] == len(members), info
        assert info["n_stored"] >= blocks[0] and info["n_fixed"] >= blocks[1] and info["n_dynamic"] >= blocks[2] + 400 and blocks[2] > 13000, (info, blocks)
        return dict(info, **z.timing())


def repeat():
    """the same input, good and corrupt members mixed (so: behind the CPU sanitizer test, as `corrupt` is), twice through one handle
    and once through a second one, a smaller input in between: identical bytes, verdicts and counters"""
    from dbg_assembly_amd import capi
    good = [m for _, ms, _ in IC.valid_groups(own=False)["zlib"] for m in IC.split(ms)]
    bad = [m for _, m, _, device_only in IC.corrupt_cases() if not device_only]
    data = b"".join(good[:8] + bad[:6] + good[8:12] + bad[6:])
    with capi.Inflater() as a, capi.Inflater() as b:
        first, i1 = a.inflate(data)
        s1 = a.member_status().tolist()
        small, _ = a.inflate(good[0])
        second, i2 = a.inflate(data)
        s2 = a.member_status().tolist()
        other, i3 = b.inflate(data)
        s3 = b.member_status().tolist()
        assert first == second == other and i1 == i2 == i3 and s1 == s2 == s3 and small == IC.verdict(good[0])
        assert a.results() == second
    return {"members": i1["n_members"], "bad": i1["n_bad"], "bytes": len(first)}


def streaming():
    """a 40-member file through Inflater.stream at window sizes that cut members inside the header, inside the stream, inside the
    trailer and exactly between members"""
    from dbg_assembly_amd import capi
    text = DC.fastq_like(40 * 700, seed=29)
    members = [IC.zmember(text[i:i + 700], (1, 6, 9, 0)[i // 700 % 4]) for i in range(0, len(text), 700)]
    data = b"".join(members) + DR.MARKER
    bounds = {0}
    for m in members + [DR.MARKER]:
        bounds.add(max(bounds) + len(m))
    first, second = len(members[0]), len(members[0]) + len(members[1])
    windows = {"inside_the_header": first + 7, "inside_the_stream": first + 100, "inside_the_trailer": second - 3, "between_members": first,
               "smaller_than_a_member": 50, "the_whole_file": len(data) + 5}
    res = {}
    with capi.Inflater() as z:
        for name, w in windows.items():
            out, cut = [], set()
            fed = 0
            for got, info in z.stream(io.BytesIO(data), w):
                out.append(got)
                assert info["n_bad"] == 0
                fed += info["consumed"]
                assert fed in bounds, (name, fed)
                cut.add(fed)
            assert b"".join(out) == text == gzip.decompress(data), name
            assert fed == len(data)
            res[name] = len(out)
        assert first + 7 not in bounds and second - 3 not in bounds and first in bounds
        res["tail_with_last"] = status_of(lambda: z.inflate(data[:first + 100], last=True))
        got, info = z.inflate(data[:first + 100], last=False)
        assert got == text[:700] and info["consumed"] == first and info["n_members"] == 1
        got, info = z.inflate(data[:10], last=False)
        assert got == b"" and info["consumed"] == 0 and info["n_members"] == 0
    return res


def max_out():
    """max_out_bytes of 1, 65 279, 65 280 and 3 * 65 280 + 1 on five full members: 0, 0, 1 and 3 members are taken"""
    from dbg_assembly_amd import capi
    text = DC.fastq_like(5 * DR.PIECE, seed=31)
    members = [IC.zmember(text[i:i + DR.PIECE]) for i in range(0, len(text), DR.PIECE)]
    data = b"".join(members)
    res = {}
    for cap, n in ((1, 0), (DR.PIECE - 1, 0), (DR.PIECE, 1), (3 * DR.PIECE + 1, 3)):
        with capi.Inflater(cap) as z:
            got, info = z.inflate(data, last=False)
            assert got == text[:n * DR.PIECE] and info["n_members"] == n and info["consumed"] == sum(len(m) for m in members[:n]), (cap, info)
            res[str(cap)] = info["n_members"]
    return res


def device_input():
    """members inside a larger device buffer through inflate_device with the table: noise in front, between and behind the members has
    no effect and the buffer is not written; a range that holds no member gets the verdict FRAME; a misaligned pointer is refused"""
    from dbg_assembly_amd import capi
    rng = np.random.default_rng(9)
    cases = [(n, m, t) for n, ms, t in IC.valid_groups(own=False)["small"] for m in IC.split(ms) for t in [IC.verdict(m)]]
    frame_case = next(m for n, m, r, device_only in IC.corrupt_cases() if device_only)
    res = {}
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Inflater() as z:
        for front in (16, 48, 4096 + 32):
            parts, off, at = [rng.integers(0, 256, front, dtype=np.uint8).tobytes()], [], front
            for _, m, _ in cases:
                parts.append(m)
                off.append(at)
                at += len(m)
            off.append(at)
            size = at + 200 + (-(at + 200) % 16)
            parts.append(rng.integers(0, 256, size - at, dtype=np.uint8).tobytes())
            host = np.frombuffer(b"".join(parts), dtype=np.uint8)
            d = g.malloc(size)
            try:
                d.from_host(host)
                got, info = z.inflate_device(d.ptr, off, size)
                want = b"".join(t for _, _, t in cases)
                assert got == want and info["n_bad"] == 0 and info["consumed"] == at and info["n_members"] == len(cases), (front, info)
                # gaps between the members: every second member alone, with the others as noise between the ranges
                pairs = [(off[i], off[i + 1]) for i in range(0, len(cases), 2)]
                outs = []
                for a, b in pairs:
                    got, info = z.inflate_device(d.ptr, [a, b], size)
                    outs.append(got)
                    assert info["n_members"] == 1 and info["n_bad"] == 0
                assert b"".join(outs) == b"".join(cases[i][2] for i in range(0, len(cases), 2))
                assert np.array_equal(d.to_host(np.uint8, size), host), "the input was written"
                # a table that points into noise, and one that points at the member which is not the framing
                got, info = z.inflate_device(d.ptr, [0, front, off[1]], size)
                assert info["n_bad"] == 1 and z.member_status().tolist() == [IC.R["FRAME"], 0] and got == cases[0][2]
                res["front_%d" % front] = len(want)
                res["misaligned"] = status_of(lambda: z.inflate_device(d.ptr + 4, [12, 12 + len(cases[0][1])], size - 4))
                res["offsets_decrease"] = status_of(lambda: z.inflate_device(d.ptr, [off[1], off[0]], size))
                res["offsets_past_the_buffer"] = status_of(lambda: z.inflate_device(d.ptr, [0, size + 1], size))
            finally:
                d.free()
        d = g.malloc(len(frame_case) + 16)
        d.from_host(np.frombuffer(frame_case, dtype=np.uint8))
        got, info = z.inflate_device(d.ptr, [0, len(frame_case)], len(frame_case))
        assert got == b"" and z.member_status().tolist() == [IC.R["FRAME"]]
        d.free()
    return res


def roundtrip():
    """Deflater at levels 0, 1 and 2 -> Inflater.inflate_device on the deflater's output where it lies -> Parser.chunk_device on the
    inflater's: the batch equals the parse of the original text"""
    from dbg_assembly_amd import capi
    import parse_cases as PC
    text = open(os.path.join(PC.CLEAN, "reads.fq"), "rb").read()
    res = {}
    with capi.Parser(PC.FASTQ, True) as p:
        want_info = p.chunk(text)
        want = [a.copy() if a is not None else None for a in p.results()]
        for level in DC.LEVELS:
            with capi.Deflater(level) as dz, capi.Inflater() as z:
                packed = dz.deflate(text)
                ptr, n = dz.device()
                off = [o for o, _, _ in DR.walk(packed)] + [len(packed)]
                got, info = z.inflate_device(ptr, off, n)
                assert got == text and info["n_bad"] == 0 and info["n_markers"] == 1
                t = z.device()
                assert t.numel() == len(text) and t.data_ptr() % 16 == 0 and bytes(t[:64].cpu().numpy()) == text[:64]
                info2 = p.chunk_device(t.data_ptr(), t.numel())
                second = p.results()
                assert all(want_info[f] == info2[f] for f in ("n_records", "n_lines", "n_bases", "mismatched", "max_len", "consumed"))
                assert all(np.array_equal(a, b) for a, b in zip(want, second)) and info2["n_records"] > 0
                res["level_%d" % level] = {"packed": len(packed), "members": info["n_members"]}
    return res


def states():
    from dbg_assembly_amd import capi
    L = capi.lib()
    res = {}
    h = ctypes.c_void_p()
    res["max_out_2_to_the_31"] = L.dbgk_inf_create(1 << 31, ctypes.byref(h))
    text = b"@r\nACGT\n+\nIIII\n"
    member = IC.zmember(text)
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g, capi.Inflater() as z:
        res["results_before_a_call"] = status_of(z.results)
        res["device_before_a_call"] = status_of(z.device_ptr)
        res["status_before_a_call"] = L.dbgk_inf_member_status(z._h, None, 0)
        res["n_bytes_2_to_the_31"] = L.dbgk_inf_inflate(z._h, member, 1 << 31, 1, ctypes.byref(capi.InfInfo()))
        res["plain_gzip"] = status_of(lambda: z.inflate(gzip.compress(text)))
        assert "16 fixed header bytes" in L.dbgk_last_error().decode()
        res["plain_text"] = status_of(lambda: z.inflate(text * 4))
        res["other_subfield"] = status_of(lambda: z.inflate(member[:12] + b"XY" + member[14:]))
        res["isize_above_a_piece"] = status_of(lambda: z.inflate(member[:-4] + struct.pack("<I", DR.PIECE + 1)))
        res["cut_short_with_last"] = status_of(lambda: z.inflate(member[:-1]))
        res["results_after_a_refused_call"] = status_of(z.results)
        d = g.malloc(len(member) + 64)
        d.from_host(np.frombuffer(member, dtype=np.uint8))
        res["n_bytes_2_to_the_31_device"] = status_of(lambda: z.inflate_device(d.ptr, [0, len(member)], 1 << 31))
        res["misaligned_input"] = status_of(lambda: z.inflate_device(d.ptr + 4, [0, 8], 8))
        res["empty_without_last"] = status_of(lambda: z.inflate(b"", last=False))
        assert z.results() == b"" and z.device_ptr() == (None, 0) and z.info["n_members"] == 0
        res["empty_with_last"] = status_of(lambda: z.inflate(b""))
        res["marker_alone"] = status_of(lambda: z.inflate(DR.MARKER))
        assert z.results() == b"" and z.info["n_members"] == 1 and z.info["n_markers"] == 1
        got, info = z.inflate_device(d.ptr, [0, len(member)])
        assert got == text
        ptr, n = z.device_ptr()
        res["own_output_as_input"] = status_of(lambda: z.inflate_device(ptr, [0, 16], 16))
        res["results_after_refused_input"] = status_of(z.results)
        out = np.zeros(n, dtype=np.uint8)
        res["capacity_one_short"] = L.dbgk_inf_results(z._h, out.ctypes.data, n - 1)
        res["capacity_exact"] = L.dbgk_inf_results(z._h, out.ctypes.data, n)
        assert out.tobytes() == got
        res["status_capacity_short"] = L.dbgk_inf_member_status(z._h, out.ctypes.data, 0)
        res["null_info"] = L.dbgk_inf_inflate(z._h, member, len(member), 1, None)
        with capi.Inflater(10) as small:
            res["device_input_above_max_out"] = status_of(lambda: small.inflate_device(d.ptr, [0, len(member)]))
        d.free()
    return res


def programs():
    """bin/clean_lowqual and bin/correct_error_reads on their golden inputs, re-framed as BGZF members by the restatement and stored
    under the goldens' names: with DBGK_GUNZIP=device outputs and .stat files equal the goldens; the same switch on the input as plain
    gzip gives the same again (the zlib path); a BGZF input with one corrupted member ends the program with status 1 and the message"""
    import clean_restatement as CR
    import test_clean_cpu as TC
    import test_correct_cpu as TO
    res = {}
    env = dict(os.environ, DBGK_GUNZIP="device")
    case = next(c for c in TC.golden_cases() if c["program"] == "clean_lowqual" and c["input"] == "reads.fq")
    want = CR.expected_outputs(TC.CASES, case)
    text = open(os.path.join(TC.CASES, case["input"]), "rb").read()
    forms = {"bgzf": DR.deflate(text, 2)[0], "plain_gzip": gzip.compress(text)}
    bad = bytearray(forms["bgzf"])
    bad[40] ^= 0x10
    forms["corrupt"] = bytes(bad)
    assert IC.verdict(forms["corrupt"]) is None
    for form, data in forms.items():
        with tempfile.TemporaryDirectory() as tmp:
            open(os.path.join(tmp, case["input"]), "wb").write(data)
            r = subprocess.run([os.path.join(TC.BIN, "clean_lowqual")] + case["args"] + [case["input"], "out.gz", "out.stat"], env=env, capture_output=True,
                               text=True, timeout=120, cwd=tmp)
            if form == "corrupt":
                assert r.returncode == 1 and "member 0" in r.stderr and case["input"] in r.stderr, (r.returncode, r.stderr[-1000:])
                res["corrupt_message"] = r.stderr.strip().splitlines()[-1]
                continue
            assert r.returncode == 0, (form, r.stderr[-2000:])
            assert gzip.decompress(open(os.path.join(tmp, "out.gz"), "rb").read()).decode("latin-1") == want["out"], form
            assert open(os.path.join(tmp, "out.stat"), "rb").read().decode("latin-1") == want["stat"], form
            res["clean_lowqual_" + form] = len(data)
    d, case = TO.golden_cases()[0]
    D = os.path.join(TO.GOLDEN, d)
    raw = open(os.path.join(D, case["reads"]), "rb").read()
    text = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
    for form, data in (("bgzf", DR.deflate(text, 2)[0]), ("plain_gzip", gzip.compress(text))):
        with tempfile.TemporaryDirectory() as tmp:
            open(os.path.join(tmp, case["reads"]), "wb").write(data)
            open(os.path.join(tmp, "reads.lib"), "w").write("%s\n" % os.path.join(tmp, case["reads"]))
            r = subprocess.run([TO.EXE] + case["args"] + [os.path.join(D, "table.cz"), os.path.join(tmp, "reads.lib")], env=env, capture_output=True, text=True,
                               timeout=120)
            assert r.returncode == 0, (form, r.stderr[-2000:])
            assert gzip.decompress(open(os.path.join(tmp, case["reads"] + ".correct.fa.gz"), "rb").read()) == TO.expected_fa(d, case), form
            assert open(os.path.join(tmp, case["reads"] + ".correct.stat"), "rb").read() == open(os.path.join(D, case["name"] + ".correct.stat"), "rb").read(), form
            res["correct_error_reads_" + form] = len(data)
    return res


if __name__ == "__main__":
    print(json.dumps({"crafted": crafted, "corrupt": corrupt, "rounds": rounds, "repeat": repeat, "streaming": streaming, "max_out": max_out,
                      "device_input": device_input, "roundtrip": roundtrip, "states": states, "programs": programs}[sys.argv[1]]()))
