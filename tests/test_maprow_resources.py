"""Register / scratch budgets of the ROWS kernels (csrc/dbgk_maprow.h), read from the built libdbgk.so (no GPU needed).  The token
kernel holds one header's cursor; the length kernel two hits and their digit counts; the segment kernel one hit, the composer's
64-bit register and a number's eight ASCII digits; the write kernel one row's six cumulative lengths and four source addresses beside
the lane's four output dwords.  64 VGPRs leave every SIMD its eight waves, like the neighbouring output kernels, and nothing may fall
into scratch -- the rule function of dbgk_maprow_rule.h returns the identity's text packed in two 64-bit registers for that reason.

The segment kernel does NOT meet 64: it is built with 95 VGPRs.  One thread holds a hit's eight numbers, the read's and the contig's
length, the composer's state and a number's digit chain, and the identity rule's 64-bit products beside them.  Its waves are bounded
by LDS before registers: a workgroup holds 256 x 112 = 28 672 bytes, so a CU's 160 KiB take five workgroups, five waves per SIMD, and
512 / 5 = 102 VGPRs (96 at the allocation granule of 8) cost no wave.  Its budget is therefore 96, the most that keeps the LDS-bound
occupancy, as for k_annot_write.

The counts are exact: one token kernel, one length kernel, one segment kernel, two forms of the write kernel (rows, FASTA).  The
kernels carry none of the name fragments the other stages' resource tests count."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, instances)
    "k_maprow_ids": (64, 1),
    "k_maprow_len": (64, 1),
    "k_maprow_num": (96, 1),   # built: 95 (the docstring says why 64 is not met and what 96 keeps)
    "k_maprow_write": (64, 2),
}
FOREIGN = ("k_map_reads", "k_fmt_", "k_emit_", "k_pair_", "k_parse_", "k_gz_", "k_annot_", "k_corr_classify", "k_corr_fix", "k_corr_overflow",
           "k_corr_seal", "k_corr_from_counts")


def test_rows_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    found = [n for n in meta if "k_maprow_" in n and not n.endswith(".kd")]
    assert len(found) == 5, found
    for n in found:
        assert not any(frag in n for frag in FOREIGN), n
    for frag, (vgprs, instances) in BUDGETS.items():
        names = [n for n in found if frag in n]
        assert len(names) == instances, (frag, names)
        for n in names:
            m = meta[n]
            print(n, m)
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
