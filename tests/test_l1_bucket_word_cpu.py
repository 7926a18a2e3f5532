"""CPU: the bucket word of the pipelined level-1 forms and the LDS layout it rests on (dbg_assembly_amd/csrc/dbgk_partition.h:
l1_bucket_word_pack / l1_bucket_word_unpack, L1PipeLds; dbgk_partition_l1.h: UniformPipeLds, PrefixPipeLds), through a small
stand-alone program (tests/l1_bucket_word_main.cpp) built with the HIP compiler, its host side under ASan + UBSan.  The program runs
alone: nothing is loaded into Python.

  the word      (entry offset << 17) | rank in bytes: every histogram entry with every rank a tile can give, the two maxima together,
                the whole width of either field against the other's edges, for both record sizes (8, and 4 for a KFREQ handle with
                direct blocks); whole words order like their entries (the test for "has no bucket")
  the layout    the packed words and the small arrays in front of the stage buffer and inside 64 KiB, lbase at one distance from both
                histograms, every histogram entry's LDS address inside the word's upper field, everything inside 160 KiB
  the library   the kernels that make LDS pointers from these offsets have no static LDS in front of their dynamic LDS
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
LIB = os.path.join(ROOT, "dbg_assembly_amd", "lib", "libdbgk.so")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "the HIP compiler is needed (as for the build)"
    exe = str(tmp_path_factory.mktemp("l1_bucket_word") / "l1_bucket_word_main")
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "dbg_assembly_amd", "csrc"),
           os.path.join(ROOT, "tests", "l1_bucket_word_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")   # (the HIP runtime's own start-up allocations are not this program's)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=env)


def fields(line):
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split()[1:])}


@pytest.mark.parametrize("rec", (8, 4))
def test_bucket_word_round_trip_over_both_fields(program, rec):
    res = run(program, ["word", str(rec)])
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    f = fields(res.stdout.splitlines()[-1])
    entries, ranks = 2 * (1024 + 64), 16 * 1024
    assert f["rec"] == rec and f["bad"] == 0
    assert f["checked"] >= entries * ranks + 5 * (1 << 15) + 10 * (1 << 17) + 3 * entries, f


def test_layout_small_arrays_first_and_in_offset_reach(program):
    res = run(program, ["layout"])
    assert res.returncode == 0, res.stderr[-2000:]
    f = fields(res.stdout.splitlines()[-1])
    assert (f["max_b"], f["threads"]) == (1024, 1024)
    assert f["hist_words"] == f["max_b"] + 64
    assert f["lbase_dist"] == 2 * f["hist_words"] * 4, "lbase lies behind both histograms, at one distance from either"
    assert f["head_bytes"] == f["lbase_dist"] + (f["hist_words"] + f["max_b"]) * 4
    assert f["head_off"] == f["prefix_head_off"] and f["head_off"] % 16 == 0
    assert f["head_off"] + 2 * f["hist_words"] * 4 <= 1 << (32 - f["rank_bits"]) and 8 * (16 * f["threads"] - 1) < 1 << f["rank_bits"]
    for form in ("uniform", "prefix"):
        stage, total = f[form + "_stage"], f[form + "_bytes"]
        assert f["head_off"] + f["head_bytes"] <= stage <= 64 * 1024 and stage % 16 == 0, form
        assert total == stage + 8 * 16 * f["threads"] <= 160 * 1024, form
        assert (stage + 8 * 16 * f["threads"]) // 8 < 1 << 16, "a run's first record travels in sixteen bits"


def group_segment_sizes(tmp_path):
    work = tmp_path / "co"
    work.mkdir()
    so = work / "libdbgk.so"
    shutil.copy(LIB, so)   # (llvm-objdump writes the bundles next to its input)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(so)], check=True, capture_output=True, cwd=work)
    sizes = {}
    for f in sorted(work.iterdir()):
        if "gfx950" not in f.name:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        size = None
        for line in notes.splitlines():   # (a kernel's fields are listed in alphabetical order: the size comes before the name)
            m = re.match(r"\s+\.group_segment_fixed_size:\s+(\d+)", line)
            if m:
                size = int(m.group(1))
            m = re.match(r"\s+\.name:\s+(\S+)", line)
            if m and size is not None:
                sizes[m.group(1)] = size
                size = None
    return sizes


def test_pipelined_kernels_have_no_static_lds(tmp_path):
    """their LDS addresses are offsets from the start of the dynamic LDS, which is LDS address 0 only without static LDS in front of it"""
    assert os.path.exists(LIB), "libdbgk.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("the ROCm LLVM tools are not installed")
    sizes = group_segment_sizes(tmp_path)
    hits = {n: s for n, s in sizes.items() if re.search(r"\d(k_extract_scatter_uniform|k_extract_scatter_prefix)I", n)}
    # every kernel of the two families, whatever their number; the flagship form and the pipelined lane-prefix form by name
    for form in ("k_extract_scatter_uniformILi0ELi0ELi15ELb0ELb0ELb1ELb1ELb1ELb1EE", "k_extract_scatter_uniformILi0ELi3ELi15ELb0ELb0ELb0ELb0ELb1ELb0EE",
                 "k_extract_scatter_prefixILi0ELi15ELb1EE"):
        assert sum(form in n for n in hits) == 1, form
    assert all(s == 0 for s in hits.values()), {n: s for n, s in hits.items() if s}
