"""CPU: the INFLATE stage without a device.  The decode core (csrc/dbgk_inflate_core.h) -- the functions the decode kernel compiles --
as a program of its own under the address and undefined-behaviour sanitizers (tests/inflate_core_test.cpp): every crafted member
(tests/inflate_cases.py), valid and corrupt, decoded out of and into heap buffers of exactly the member's sizes, bytes and verdict
compared with zlib's, block and token counters and the largest distance with the token lister's (tests/deflate_tokens.py), each
reason code reached; 2 000 damaged members within the bound on loop iterations.  Then the INFLATE
section's symbols, reason codes and struct sizes in header and binding, and the argument checks that need no device.  Every test
here fails without the stage: the core, the section and capi.Inflater do not exist."""
import ctypes as C
import gzip
import os
import re
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_cases as IC  # noqa: E402
from dbg_assembly_amd import capi  # noqa: E402

NAMES = ("dbgk_inf_create", "dbgk_inf_destroy", "dbgk_inf_inflate", "dbgk_inf_inflate_device", "dbgk_inf_results", "dbgk_inf_device",
         "dbgk_inf_member_status", "dbgk_inf_timing_get")
SAN = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
       "-static-libubsan"]
N_DAMAGED = 2000


def compiler():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no system C++ compiler"
    return cxx


def test_the_decode_core_under_the_sanitizers_agrees_with_zlib_on_every_crafted_member(tmp_path):
    exe = tmp_path / "inflate_core_test"
    subprocess.run([compiler()] + SAN + ["-I" + os.path.join(ROOT, "dbg_assembly_amd", "csrc"), os.path.join(ROOT, "tests", "inflate_core_test.cpp"),
                                         "-o", str(exe), "-lz"], check=True, timeout=180)
    rows = []   # (name, member, zlib's bytes or None, reason expected of a corrupt one, the lister's (counters, largest distance) or None)
    for group, cases in IC.valid_groups().items():
        for name, members, text in cases:
            assert gzip.decompress(members) == text, name   # (concatenated members are one gzip file)
            for m in IC.split(members):
                want = IC.verdict(m)
                assert want is not None, name
                rows.append((name, m, want, 0, IC.listed(m)))
    corrupt = IC.corrupt_cases()
    for name, m, reason, _ in corrupt:
        assert IC.verdict(m) is None, "zlib accepts %s" % name
        rows.append((name, m, None, reason, None))
    assert {r for _, _, r, _ in corrupt} == set(range(1, len(IC.REASONS))), "a reason code that no case reaches"
    with open(tmp_path / "cases.bin", "wb") as f:
        for _, m, _, _, _ in rows:
            f.write(struct.pack("<I", len(m)) + m)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(N_DAMAGED)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(rows) + 1
    got = {}
    for (name, m, want, reason, counters), line in zip(rows, lines):
        verdict, adler, n_stored, n_fixed, n_dynamic, n_literals, n_matches, far = map(int, line.split())
        assert (verdict == 0) == (want is not None), (name, verdict)
        if want is None:
            assert verdict == reason, (name, IC.REASONS[verdict], IC.REASONS[reason])
            continue
        assert adler == zlib.adler32(want), name
        found = dict(n_stored=n_stored, n_fixed=n_fixed, n_dynamic=n_dynamic, n_literals=n_literals, n_matches=n_matches)
        assert (found, far) == counters, (name, found, far, counters)
        got.setdefault(name, dict(found, far=far))   # (the first member of a case)
    # the cases sit where their names claim
    assert got["many_blocks"]["n_dynamic"] >= 200 and got["many_blocks_small"]["n_dynamic"] >= 10
    # zlib's level 0 ends the piece's stored block with an empty final one; the project's own level 0 writes the one block alone
    assert got["stored_one_block"] == dict(n_stored=2, n_fixed=0, n_dynamic=0, n_literals=IC.PIECE, n_matches=0, far=0)
    assert got["fastq_len_%d_level_0" % IC.PIECE] == dict(n_stored=1, n_fixed=0, n_dynamic=0, n_literals=IC.PIECE, n_matches=0, far=0)
    assert got["fixed_codes"]["n_fixed"] >= 1 and got["fixed_codes"]["n_dynamic"] == 0 and got["fixed_small"]["n_fixed"] == 1
    assert got["one_value_zlib_9"]["n_matches"] >= (IC.PIECE - 3) // 258 and got["one_value_zlib_9"]["n_literals"] <= 3   # length 258 at distance 1
    assert got["random_zlib_6"]["n_stored"] >= 1 and got["empty_stored_blocks"] == dict(n_stored=3, n_fixed=1, n_dynamic=0, n_literals=2, n_matches=0, far=0)
    assert got["single_distance_symbol"]["n_matches"] == 2 and got["no_distance_code"]["n_matches"] == 0
    assert all(got["flush_at_%d" % p]["n_stored"] == 2 for p in (1,))
    assert got["fibonacci_counts_with_eob_level_1"]["n_dynamic"] == 1   # a 15-bit code
    # distances: zlib reaches 32 506 at the most (its window less its look-ahead), so the repeat of a 32 768-byte block gives it no
    # match; the project's own members and the hand-made one hold the far ones, up to distance symbol 29 with every extra bit set
    assert got["distance_32768_zlib_9"]["n_matches"] == 0
    assert got["distance_32768_level_2"]["far"] == 32768 and got["distance_24577_level_2"]["far"] == 24577
    assert got["matches_at_32768_and_32767"] == dict(n_stored=1, n_fixed=1, n_dynamic=0, n_literals=32768, n_matches=2, far=32768)
    assert (100, 32767) in IC.DT.gzip_member(IC.far_match_member()[0])[0][1]["tokens"]
    assert max(v["far"] for v in got.values()) == 32768
    m = re.match(r"damaged (\d+) refused (\d+) worst (\d+) of (\d+)", lines[-1])
    assert m and int(m.group(1)) == N_DAMAGED and int(m.group(2)) > N_DAMAGED // 2 and int(m.group(3)) <= int(m.group(4))


def test_header_and_binding_agree(tmp_path):
    L = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    for name in NAMES:
        assert hasattr(L, name), "libdbgk.so does not export %s" % name
        assert name in bound and bound[name][1] is C.c_int, name
    header = open(os.path.join(ROOT, "include", "dbgk.h")).read()
    defined = {n: int(v) for n, v in re.findall(r"#define DBGK_INF_([A-Z_]+) (\d+)", header)}
    assert defined.pop("ROUND") == capi.INF_ROUND
    assert defined == IC.R == {n: i for i, n in enumerate(capi.INF_REASONS)}
    assert "#define DBGK_ABI_VERSION 7" in header and capi.lib().dbgk_abi_version() == 7
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include "dbgk.h"\nint main() { printf("%zu %zu\\n", sizeof(dbgk_inf_info), sizeof(dbgk_inf_timing)); }\n')
    subprocess.run([compiler(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")], check=True, timeout=120)
    sizes = subprocess.run([str(tmp_path / "sizes")], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in sizes] == [C.sizeof(capi.InfInfo), C.sizeof(capi.InfTiming)] == [96, 24]
    for f in ("inflate", "inflate_device", "device", "results", "member_status", "timing", "stream"):
        assert callable(getattr(capi.Inflater, f))


def test_the_argument_checks_that_need_no_device():
    """The checks of n_bytes >= 2^31 and of bytes that are not the framing stand behind the check of the handle, and a handle exists
    only on a device: here every call is refused for its null handle or pointer, and those two checks are made on a live handle
    by the `states` step of tests/test_inflate_gpu.py."""
    L = capi.lib()
    h = C.c_void_p()
    assert L.dbgk_inf_create(0, None) == capi.ERR_ARG
    assert L.dbgk_inf_create(1 << 31, C.byref(h)) == capi.ERR_ARG and not h.value
    info, t, p, n = capi.InfInfo(), capi.InfTiming(), C.c_void_p(), C.c_uint64()
    buf = np.frombuffer(IC.DR.MARKER, dtype=np.uint8).copy()
    off = (C.c_uint64 * 2)(0, 28)
    assert L.dbgk_inf_inflate(None, buf.ctypes.data, 28, 1, C.byref(info)) == capi.ERR_ARG
    assert L.dbgk_inf_inflate_device(None, None, 0, off, 1, C.byref(info)) == capi.ERR_ARG
    assert L.dbgk_inf_results(None, buf.ctypes.data, 28) == capi.ERR_ARG
    assert L.dbgk_inf_device(None, C.byref(p), C.byref(n)) == capi.ERR_ARG
    assert L.dbgk_inf_member_status(None, buf.ctypes.data, 28) == capi.ERR_ARG
    assert L.dbgk_inf_timing_get(None, C.byref(t)) == capi.ERR_ARG
    assert L.dbgk_inf_destroy(None) == capi.ERR_ARG
    if L.dbgk_device_count() == 0:   # no fall-back to zlib: the library's error
        assert L.dbgk_inf_create(0, C.byref(h)) == capi.ERR_HIP and not h.value
        with pytest.raises(capi.DbgkError):
            capi.Inflater()
