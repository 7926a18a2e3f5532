"""Register / scratch budgets of the link_contig kernels, read from the built libdbgk.so (no GPU needed).  None of them may use
scratch.  The orient forms, the gather, the gap statistics and the emit kernel are streaming kernels of 256 threads and get the 64
VGPRs of their link_scaffold siblings (eight waves per SIMD).  The consensus kernel keeps five counters, the descriptor of its gap
and the slice addresses of a round of reads in registers: the build reports 42 VGPRs, and the budget is the next occupancy step
above that, 48 (ten waves per SIMD of 512 VGPRs)."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, forms)
    "k_fill_orient": (64, 2),      # from records and from mapper hits
    "k_fill_gather": (64, 1),
    "k_fill_gapstat": (64, 1),
    "k_fill_consensus": (48, 1),
    "k_fill_emit": (64, 1),
}


def test_fill_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, (vgprs, forms) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) >= forms, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
    assert len([n for n in meta if "k_fill_" in n and not n.endswith(".kd")]) == 6
