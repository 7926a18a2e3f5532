"""CPU: the DEFLATE stage without a device.  The token lister (tests/deflate_tokens.py) against zlib's own streams; the restatement of
the stage's rules (tests/deflate_restatement.py) against gzip.decompress, which checks CRC-32 and ISIZE; the framing header
(csrc/dbgk_gz_frame.h) as a program of its own under the address and undefined-behaviour sanitizers (tests/gz_frame_test.cpp) and
through the restatement's member list; every crafted case (tests/deflate_cases.py) where its name claims; the match cases by the level-2 parse; the GZ section's symbols,
struct sizes and the argument checks that need no device."""
import ctypes as C
import gzip
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_cases as DC  # noqa: E402
import deflate_restatement as DR  # noqa: E402
import deflate_tokens as DT  # noqa: E402
from dbg_assembly_amd import capi  # noqa: E402

DC_CASES = DC.cases()
NAMES = ("dbgk_gz_create", "dbgk_gz_destroy", "dbgk_gz_deflate", "dbgk_gz_deflate_device", "dbgk_gz_results", "dbgk_gz_device", "dbgk_gz_timing_get")


@pytest.fixture(scope="module")
def restated():
    """{(name, level): (bytes, info, [(member, stored, parts)])}, computed once"""
    out = {}
    for name, data in DC_CASES.items():
        for level in DC.LEVELS:
            out[name, level] = DR.deflate(data, level) + (DR.members(data, level),)
    return out


def test_the_token_lister_reproduces_zlib_on_stored_fixed_and_dynamic_blocks():
    text = DC.fastq_like(20000)
    seen = set()
    for data, level, strategy in ((text, 0, zlib.Z_DEFAULT_STRATEGY), (text[:70], 6, zlib.Z_FIXED), (text, 6, zlib.Z_DEFAULT_STRATEGY),
                                  (text, 1, zlib.Z_DEFAULT_STRATEGY), (text, 6, zlib.Z_HUFFMAN_ONLY), (b"A" * 3000, 9, zlib.Z_DEFAULT_STRATEGY),
                                  (b"", 6, zlib.Z_DEFAULT_STRATEGY), (bytes(range(256)) * 3, 6, zlib.Z_RLE)):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        raw = c.compress(data) + c.flush()
        blocks, out, used = DT.blocks(raw)
        assert out == data == zlib.decompress(raw, -15) and (used + 7) // 8 == len(raw)
        for b in blocks:
            seen.add(b["type"])
            assert sum(1 if isinstance(t, int) else t[0] for t in b["tokens"]) <= len(data)
        assert sum(1 if isinstance(t, int) else t[0] for b in blocks for t in b["tokens"]) == len(data)
    assert seen == {"stored", "fixed", "dynamic"}
    blocks, _, _ = DT.blocks(zlib.compress(b"A" * 3000, 9)[2:-4])
    assert (258, 1) in blocks[0]["tokens"]
    for bad in (b"\x07", b"\x01\x01\x00\x00\x00", b"\x05"):   # reserved type, a stored length check that fails, a dynamic block cut short
        with pytest.raises(ValueError):
            DT.blocks(bad)


def test_the_restatement_gives_gzip_members_that_inflate_to_the_input(restated):
    for (name, level), (out, info, ms) in restated.items():
        data = DC_CASES[name]
        assert gzip.decompress(out) == data, (name, level)
        assert out.endswith(DR.MARKER) and info["out_bytes"] == len(out) and info["n_members"] == -(-len(data) // DR.PIECE), (name, level)
        if level == 0:
            assert info["stored_members"] == info["n_members"] and info["n_literals"] == 0
        else:
            assert len(out) <= len(restated[name, 0][0]), name
        assert DR.deflate(data, level, last=False)[0] == out[:-28]
    assert restated["empty", 1][0] == DR.MARKER and DR.deflate(b"", 1, last=False)[0] == b""


def test_the_members_are_what_the_rules_say(restated):
    """a few members through the token lister: one dynamic block with BFINAL, 257 literal lengths, one distance length 0, complete
    codes (the lister refuses others), literals only, the trailer right behind the block"""
    for name in ("fastq_len_600", "one_value", "fibonacci_counts", "cl_deeper_than_7", "two_values", "all_256_values", "fastq_len_3"):
        for member, stored, parts in restated[name, 1][2]:
            blocks, out, crc, isize = DT.gzip_member(member)
            assert len(blocks) == 1 and blocks[0]["final"] == 1 and crc == zlib.crc32(out) and isize == len(out)
            assert blocks[0]["type"] == ("stored" if stored else "dynamic")
            if not stored:
                b = blocks[0]
                assert len(b["lit_lens"]) == 257 and b["dist_lens"] == [0] and all(isinstance(t, int) for t in b["tokens"])
                assert b["lit_lens"] == parts["lens"] and b["cl_lens"] == parts["cl_lens"] and b["cl_tokens"] == parts["tokens"]
                assert max(b["lit_lens"]) <= 15 and max(b["cl_lens"]) <= 7 and sum(1 for l in b["cl_lens"] if l) >= 2


def test_the_frame_walk_agrees_with_the_member_list(restated):
    for (name, level), (out, info, ms) in restated.items():
        got = DR.walk(out)
        want, at = [], 0
        for (member, _, _), n in zip(ms, [min(DR.PIECE, len(DC_CASES[name]) - i * DR.PIECE) for i in range(len(ms))]):
            want.append((at, len(member), n))
            at += len(member)
        want.append((at, 28, 0))
        assert got == want, (name, level)
    for bad in (restated["fastq_len_600", 1][0][:-1], b"\x1f\x8b\x08\x00" + bytes(40), restated["fastq_len_600", 1][0][:16] + b"\x05\x00" + bytes(30)):
        with pytest.raises(ValueError):
            DR.walk(bad)


def test_every_case_sits_where_it_claims(restated):
    def parts(name, i=0):
        return restated[name, 1][2][i][2]

    def stored(name, i=0):
        return restated[name, 1][2][i][1]

    for n in (0, 1, 2, 3, 600, DR.PIECE - 1, DR.PIECE, DR.PIECE + 1, 2 * DR.PIECE, 2 * DR.PIECE + 1):
        assert len(DC_CASES["fastq_len_%d" % n]) == n
    assert [len(DC_CASES[n]) for n in ("empty", "one_byte", "two_bytes", "three_bytes")] == [0, 1, 2, 3]
    assert restated["fastq_len_%d" % (2 * DR.PIECE + 1), 1][1]["n_members"] == 3 and restated["fastq_len_%d" % DR.PIECE, 1][1]["n_members"] == 1
    for k in (3, 100, 200, DC.BLOCK - 1):
        assert [len(DC_CASES["slices_%d%+d" % (k, d)]) - k * DC.LANE for d in (-1, 0, 1)] == [-1, 0, 1]
    assert DC.LANE * DC.BLOCK == DR.PIECE
    # one value: a two-symbol literal code
    p = parts("one_value")
    assert [l for l in p["lens"] if l] == [1, 1] and not stored("one_value") and len(restated["one_value", 1][0]) < 8300
    # random bytes: stored, and counted
    assert restated["random_bytes", 1][1]["stored_members"] == 2 and restated["random_bytes", 1][0] == restated["random_bytes", 0][0]
    i = restated["random_then_text", 1][1]
    assert (i["n_members"], i["stored_members"], i["n_literals"]) == (2, 1, 5000)
    # length limiting, literals: 22 values with Fibonacci counts
    p = parts("fibonacci_counts")
    assert len(DC_CASES["fibonacci_counts"]) == 46367 and sum(1 for f in p["freq"] if f) == 23
    assert max(DR.unlimited_depths(sorted(f for f in p["freq"] if f))) == 12 == max(p["lens"])   # ties go to the leaf: no chain
    p = parts("fibonacci_counts_with_eob")
    assert len(DC_CASES["fibonacci_counts_with_eob"]) == 46366 and sum(1 for f in p["freq"] if f) == 22
    assert max(DR.unlimited_depths(sorted(f for f in p["freq"] if f))) == 21 and max(p["lens"]) == 15 and not stored("fibonacci_counts_with_eob")
    assert sorted(l for l in p["lens"] if l) != sorted(min(d, 15) for d in DR.unlimited_depths(sorted(f for f in p["freq"] if f)))
    # length limiting, the code of the length sequence
    p = parts("cl_deeper_than_7")
    assert max(DR.unlimited_depths(sorted(f for f in p["cl_freq"] if f))) == 8 and max(p["cl_lens"]) == 7 and not stored("cl_deeper_than_7")
    assert max(p["lens"]) == 15 and p["hclen"] == 19
    # runs of lengths
    t = [s for s, _ in parts("two_values")["tokens"]]
    assert (18, 127) in parts("two_values")["tokens"] and 17 in t and sum(1 for l in parts("two_values")["lens"] if l) == 3
    t = parts("all_256_values")["tokens"]
    assert (16, 3) in t and [s for s, _ in t].count(16) > 30
    assert sum(1 for l in parts("all_256_values")["lens"] if l) == 257
    # HCLEN at both ends; a dynamic block that is not smaller
    p = parts("255_values_once")
    assert p["hclen"] == 5 and p.get("rejected") and stored("255_values_once") and set(p["lens"][:255]) == {8}
    assert parts("fibonacci_counts_with_eob")["hclen"] == 19
    # bit placement: the second lane starts at every residue mod 64, so on a byte, a dword and a qword boundary too
    starts = set()
    for k in range(1, 64):
        name = "second_lane_starts_%d_bits_later" % k
        p = parts(name)
        assert not stored(name) and [p["lens"][ord("a")], p["lens"][ord("b")], p["lens"][256]] == [1, 2, 2]
        first = DC_CASES[name][:DC.LANE]
        starts.add((18 * 8 + p["head_bits"] + sum(p["lens"][b] for b in first)) % 64)
        assert len(DC_CASES[name]) == 2 * DC.LANE + 90   # a third lane with 90 tokens, 253 lanes with none
    assert len(starts) == 63 and {0, 8, 32} <= starts
    text, n = DC.rounds_text()
    assert -(-len(text) // DR.PIECE) == n > 8 * 304 and len(text) % DR.PIECE == 5


def test_the_match_cases_produce_the_matches_they_are_built_for(restated):
    """level 2, by the restatement's parse; the token lister reads the same tokens back out of the members"""
    def matches(name):
        return [t for _, stored, p in restated[name, 2][2] if not stored for t in p["parse"] if not isinstance(t, int)]

    for n in (3, 4, 257, 258):
        assert (n, 1000) in matches("match_of_%d" % n)
    got = matches("run_lengths_3_to_258")
    assert {n for n, d in got if d == 1} >= set(range(3, 259)) and restated["run_lengths_3_to_258", 2][2][0][2]["hlit"] == 286
    assert [t for t in matches("runs_of_259_and_261") if t[1] == 1] == [(258, 1), (258, 1), (3, 1)]   # 259: a literal, 258, a literal
    for k, base in enumerate(DC.DIST_BASE):
        for d in {base, (DC.DIST_BASE[k + 1] if k < 29 else 32769) - 1} - {1}:
            assert (12, d) in matches("distance_%d" % d), d
            assert DR.dist_symbol(d)[0] == k
    assert restated["distance_32768", 2][2][0][2]["hdist"] == 30 and (12, 32768) in matches("distance_32768")
    assert all(d <= 32768 and n != 12 for n, d in matches("distance_32769"))   # one byte too far: literals
    # a match whose second copy starts five bytes in front of a chunk boundary of the matcher
    text = DC_CASES["match_across_a_chunk_boundary"]
    assert (20, 1000) in matches("match_across_a_chunk_boundary") and text.index(text[19:39], 20) % DC.CHUNK == DC.CHUNK - 5
    # the second copy is cut by the end of the piece: 10 of its 50 bytes
    assert restated["match_cut_by_the_end", 2][2][0][2]["parse"][-1] == (10, 512)
    # the 40 bytes in front of the member boundary repeat behind it: the second member starts with literals
    ms = restated["repeat_across_the_member_boundary", 2][2]
    assert len(ms) == 2 and isinstance(ms[1][2]["parse"][0], int)
    assert DT.gzip_member(ms[1][0])[1] == DC_CASES["repeat_across_the_member_boundary"][DR.PIECE:]   # (the lister refuses a distance in front of the member)
    assert DC_CASES["repeat_across_the_member_boundary"][DR.PIECE - 40:DR.PIECE] == DC_CASES["repeat_across_the_member_boundary"][DR.PIECE:DR.PIECE + 40]
    # one value: a literal and a chain of 258-matches at distance 1, one distance symbol of length 1
    p = restated["one_value", 2][2][0][2]
    assert p["parse"][0] == ord("A") and set(p["parse"][1:-1]) == {(258, 1)} and [l for l in p["dlens"] if l] == [1] and p["hdist"] == 1
    assert restated["fastq_len_3", 2][2][0][2] is None or restated["fastq_len_3", 2][2][0][2]["hlit"] == 257
    # token counts around the lanes' slices of 1 and 2 tokens
    assert [len(restated["sixteen_values_%d" % n, 2][2][0][2]["parse"]) for n in (255, 256, 257)] == [255, 256, 257]
    assert 256 < len(restated["sixteen_values_513", 2][2][0][2]["parse"]) < 512
    for name in ("match_of_258", "distance_32768", "run_lengths_3_to_258", "one_value", "fastq_len_600", "match_cut_by_the_end"):
        for member, stored, parts in restated[name, 2][2]:
            blocks, out, crc, isize = DT.gzip_member(member)
            assert not stored and blocks[0]["tokens"] == parts["parse"] and crc == zlib.crc32(out)
            assert blocks[0]["lit_lens"] == parts["lens"][:parts["hlit"]] and blocks[0]["dist_lens"] == parts["dlens"][:parts["hdist"]]
    for n in range(3, 259):   # the symbol arithmetic against the tables of RFC 1951
        s, e, x = DR.len_symbol(n)
        assert DT.LEN_BASE[s - 257] + x == n and DT.LEN_EXTRA[s - 257] == e
    for d in list(range(1, 600)) + [1024, 1025, 4096, 24576, 24577, 32767, 32768]:
        s, e, x = DR.dist_symbol(d)
        assert DT.DIST_BASE[s] + x == d and DT.DIST_EXTRA[s] == e


def test_the_framing_header_under_the_sanitizers(tmp_path):
    """csrc/dbgk_gz_frame.h, compiled with the system C++ compiler and -fsanitize=address,undefined into a program with its own main
    and run as such"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no system C++ compiler"
    exe = tmp_path / "gz_frame_test"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "dbg_assembly_amd", "csrc"),
                    os.path.join(ROOT, "tests", "gz_frame_test.cpp"), "-o", str(exe), "-lz"], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("cases ok") and int(r.stdout.split()[0]) >= 100


def test_the_library_exports_the_section_and_the_binding_has_it():
    L = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    for name in NAMES:
        assert hasattr(L, name), "libdbgk.so does not export %s" % name
        assert name in bound and bound[name][1] is C.c_int, name
    assert C.sizeof(capi.GzInfo) == 6 * 8 and C.sizeof(capi.GzTiming) == 6 * 8
    assert capi.GZ_PIECE == DR.PIECE == DC.PIECE and capi.GZ_MAX_LEVEL == DR.MAX_LEVEL == max(DC.LEVELS)
    header = open(os.path.join(ROOT, "include", "dbgk.h")).read()
    assert "#define DBGK_GZ_PIECE %d" % capi.GZ_PIECE in header and "#define DBGK_GZ_MAX_LEVEL %d" % capi.GZ_MAX_LEVEL in header
    for f in ("stream", "deflate", "deflate_device", "results", "device", "timing"):
        assert callable(getattr(capi.Deflater, f))


def test_the_argument_checks_that_need_no_device():
    L = capi.lib()
    h = C.c_void_p()
    for level in (-1, capi.GZ_MAX_LEVEL + 1, 9):
        assert L.dbgk_gz_create(level, C.byref(h)) == capi.ERR_ARG and not h.value
    assert L.dbgk_gz_create(1, None) == capi.ERR_ARG
    info, t, p, n = capi.GzInfo(), capi.GzTiming(), C.c_void_p(), C.c_uint64()
    buf = np.zeros(16, dtype=np.uint8)
    assert L.dbgk_gz_deflate(None, buf.ctypes.data, 16, 1, C.byref(info)) == capi.ERR_ARG
    assert L.dbgk_gz_deflate_device(None, None, 0, 1, C.byref(info)) == capi.ERR_ARG
    assert L.dbgk_gz_results(None, buf.ctypes.data, 16) == capi.ERR_ARG
    assert L.dbgk_gz_device(None, C.byref(p), C.byref(n)) == capi.ERR_ARG
    assert L.dbgk_gz_timing_get(None, C.byref(t)) == capi.ERR_ARG
    assert L.dbgk_gz_destroy(None) == capi.ERR_ARG
    if L.dbgk_device_count() == 0:   # no fall-back to zlib: the library's error
        assert L.dbgk_gz_create(1, C.byref(h)) == capi.ERR_HIP
