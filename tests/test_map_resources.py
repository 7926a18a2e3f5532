"""Register / scratch budgets of the map_reads / map_pair kernels, read from the built libdbgk.so (no GPU needed).
The read lives in LDS or global memory, indexed by lane; none of it may fall into scratch."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> max VGPRs
    "k_map_reads": 128,
}


def test_map_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, vgprs in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) >= 2, (frag, names)  # the LDS form and the long-read form
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] <= vgprs, (n, m)
