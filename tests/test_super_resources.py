"""Register / scratch budgets of the link_supertig kernels, read from the built libdbgk.so (no GPU needed).  None of them may use
scratch.  The two passes of the segmented reduce, the pack kernel and the slice copy are streaming kernels of 256 threads and get
the 64 VGPRs of their link_scaffold and link_contig siblings (eight waves per SIMD)."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, forms)
    "k_super_gapstat": (64, 2),    # pass 0: sum, min, max, count; pass 1: deviations around the truncated mean
    "k_super_gappack": (64, 1),
    "k_super_slices": (64, 1),
}


def test_super_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, (vgprs, forms) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == forms, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
    assert len([n for n in meta if "k_super_" in n and not n.endswith(".kd")]) == 4
