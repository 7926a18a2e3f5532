"""Register / scratch budget of the kernel that aligns the bubble arms, read from the built libdbgk.so (no GPU needed).

k_align_pairs runs one wave per workgroup on 19992 bytes of LDS (the 2-bit directions of 256 x 256 cells and four small buffers), so
a CU of 160 KiB holds eight of its waves, two per SIMD, whatever its registers: occupancy is set by LDS.  The budget is there so that a
spill, or state that has no business in the kernel, is noticed.  What the kernel keeps: per step of the sweep the lane's left and
diagonal scores, the score and the character that come down from the lane above, the two values lane 0 fetched ahead, the row's
character, the 16 directions being packed, the address of the row's direction words, row, column, step and bounds (about 20); around it
the pair's six 64-bit pointers and three offsets (18) and the loop over pairs (4).  The three loops that stage the sequences and the
loop that writes the alignment out are unrolled eightfold by the compiler, which keeps eight loads with their 64-bit addresses and LDS
addresses in flight (about 40).  That is about 82; the budget is 96 -- still five waves per SIMD, more than twice what the LDS admits --
and no scratch."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {"k_align_pairs": 96}   # kernel name fragment -> max VGPRs


def test_align_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, vgprs in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == 1, (frag, names)
        m = meta[names[0]]
        print(names[0], m["vgpr_count"], m.get("agpr_count", 0), m.get("private_segment_fixed_size", 0))
        assert m.get("private_segment_fixed_size", 0) == 0, (names[0], m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (names[0], m)
    aligners = [n for n in meta if "k_align_" in n and not n.endswith(".kd")]
    assert len(aligners) == len(BUDGETS)
    # the budget tests of the traced paths and of the read-out count their kernels by these fragments
    assert not any(f in n for n in aligners for f in ("k_simp_", "k_wsimp_", "k_contig_"))
