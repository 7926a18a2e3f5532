"""Register / scratch budgets of the INFLATE stage's kernels (csrc/dbgk_inflate.h), read from the built libdbgk.so (no GPU needed).
The count is exact: sizes, decode, resolve.  A decoder keeps its tables, the lengths it reads and the arrays of the table
construction in LDS and indexes nothing in registers by a variable, so nothing may fall into scratch; 128 VGPRs keep four waves per
SIMD.  k_inf_decode is launched as one wave, the two others with 256 threads.  The reader is this file's own: it needs a kernel's
whole entry, the workgroup size stands in front of the name there."""
import os
import re
import shutil
import subprocess

from test_kernel_resources import LIB, LLVM

BUDGETS = {   # kernel name fragment -> (max VGPRs, workgroup size)
    "k_inf_sizes": (128, 256),
    "k_inf_decode": (128, 64),
    "k_inf_resolve": (128, 256),
}
KEYS = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "max_flat_workgroup_size")


def inflate_kernels(work):
    """the figures of every k_inf_ kernel out of libdbgk.so's gfx950 code objects.  A kernel's entry of the notes is read as a whole:
    some of its keys stand in front of its .name, some behind"""
    so = work / "libdbgk.so"
    shutil.copy(LIB, so)   # (llvm-objdump writes the bundles next to its input)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(so)], check=True, capture_output=True, cwd=work)
    meta = {}
    for f in sorted(work.iterdir()):
        if "gfx950" not in f.name:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        for entry in re.split(r"(?m)^  - (?=\.)", notes):
            name = re.search(r"(?m)^    \.name:\s+(\S+)", entry)
            if name and "k_inf_" in name.group(1):
                meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"(?m)^    \.(%s):\s+(\d+)" % "|".join(KEYS), entry)}
    return meta


def test_inflate_stage_kernels_fit(tmp_path):
    meta = inflate_kernels(tmp_path)
    assert len(meta) == 3, sorted(meta)
    for frag, (vgprs, block) in BUDGETS.items():
        names = [n for n in meta if frag in n]
        assert len(names) == 1, (frag, names)
        m = meta[names[0]]
        assert m["private_segment_fixed_size"] == 0, (names[0], m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (names[0], m)
        assert m["max_flat_workgroup_size"] == block, (names[0], m)
