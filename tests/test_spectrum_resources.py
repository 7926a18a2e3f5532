"""Register, scratch and LDS budgets of the two table scans of dbgk_spectrum.h, read from the built libdbgk.so (no GPU
needed).  k_kf_spectrum keeps 8 copies of the 256 bins per wave in LDS (4 waves x 8 x 256 x 4 bytes); k_mut_scan keeps
32 64-bit bins per workgroup.  Neither may spill: the scan's k windows are unrolled into registers."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM

KERNELS = {   # kernel name fragment -> (max VGPRs, LDS bytes as built)
    "k_kf_spectrum": (128, 4 * 8 * 256 * 4),
    "k_mut_scan": (128, 32 * 8),
}
FIELDS = r"\.(vgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)"


def descriptors(tmp_path):
    """the notes of the gfx950 code object, with the LDS size that test_kernel_resources.kernel_metadata leaves out"""
    work = tmp_path / "co"
    work.mkdir()
    so = work / "libdbgk.so"
    shutil.copy(LIB, so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(so)], check=True, capture_output=True, cwd=work)
    meta = {}
    for f in sorted(work.iterdir()):
        if "gfx950" not in f.name:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        block = {}
        for line in notes.splitlines() + ["  - .end:"]:
            if re.match(r"  - \.", line):   # the next kernel's entry begins: the fields before AND after .name belong to one kernel
                if "name" in block:
                    meta[block.pop("name")] = block
                block = {}
            m = re.match(r"(?:    |  - )\.name:\s+(\S+)", line)
            if m:
                block["name"] = m.group(1)
            m = re.match(r"(?:    |  - )" + FIELDS, line)
            if m:
                block[m.group(1)] = int(m.group(2))
    return meta


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="the ROCm LLVM tools are not installed")
def test_spectrum_kernels_fit(tmp_path):
    assert os.path.exists(LIB), "libdbgk.so not built"
    meta = descriptors(tmp_path)
    for frag, (vgprs, lds) in KERNELS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert names, frag
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m["group_segment_fixed_size"] == lds, (n, m)
