"""Register / scratch budgets of the link_scaffold kernels, read from the built libdbgk.so (no GPU needed).  All four are
streaming kernels of 256 threads with nothing indexed at run time: none of them may use scratch, and 64 VGPRs (what the build
leaves room for: it allocates well under half of that) keep eight waves per SIMD."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, forms)
    "k_link_orient": (64, 2),      # from records and from mapper hits
    "k_link_reduce": (64, 1),
    "k_link_chain": (64, 1),
    "k_link_emit": (64, 1),
}


def test_link_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, (vgprs, forms) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) >= forms, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
