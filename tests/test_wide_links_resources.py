"""Resources of k_wide_kmer_links (the contig stage's first pass on 32-byte nodes), read from the built libdbgk.so (no GPU needed).
Registers and scratch come from test_kernel_resources.kernel_metadata; that reader keeps no LDS size, so the static LDS of the two
kernels and of their 64-bit counterpart is read here from the same notes of the same code objects."""
import os
import re
import shutil
import subprocess

from test_kernel_resources import LIB, LLVM, kernel_metadata


def lds_sizes(tmp_path):
    """kernel name -> .group_segment_fixed_size (the notes list a kernel's keys in alphabetical order: the size comes before the name)"""
    work = tmp_path / "lds"
    work.mkdir()
    shutil.copy(LIB, work / "libdbgk.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "libdbgk.so"], check=True, capture_output=True, cwd=work)
    out = {}
    for f in sorted(work.iterdir()):
        if "gfx950" not in f.name:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        size = None
        for line in notes.splitlines():
            m = re.match(r"\s+\.group_segment_fixed_size:\s+(\d+)", line)
            if m:
                size = int(m.group(1))
            m = re.match(r"\s+\.name:\s+(\S+)", line)
            if m and size is not None:
                out[m.group(1)] = size
                size = None
    return out


def test_wide_link_kernels_fit(tmp_path):
    """Both instantiations: no scratch; at most 64 VGPRs -- a streaming kernel of 256 threads whose time goes into loads, which wants
    the eight waves per SIMD that 64 registers still give (the budget of the other streaming kernels); static LDS no larger than
    k_kmer_links' own (the same histogram, wave counts and running sums)."""
    meta = kernel_metadata(tmp_path)
    lds = lds_sizes(tmp_path)
    for p in (0, 1):
        wide = [n for n in meta if "k_wide_kmer_linksILi%dE" % p in n and not n.endswith(".kd")]
        narrow = [n for n in meta if "12k_kmer_linksILi%dE" % p in n and not n.endswith(".kd")]
        assert len(wide) == 1 and len(narrow) == 1, (p, wide, narrow)
        m = meta[wide[0]]
        assert m.get("private_segment_fixed_size", 0) == 0, (wide[0], m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= 64, (wide[0], m)
        assert lds[wide[0]] <= lds[narrow[0]], (wide[0], lds[wide[0]], lds[narrow[0]])
