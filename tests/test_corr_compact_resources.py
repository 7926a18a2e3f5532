"""Register / scratch budgets of the corrector's output-stage kernels, read from the built libdbgk.so (no GPU needed).
The gather keeps a tile, a list of reads and two search results in LDS; a lane holds one 16-byte vector, a few offsets and
the counters of the length kernel: 64 VGPRs leave every SIMD its eight waves, and nothing may fall into scratch."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> max VGPRs
    "k_corr_out_len": 64,
    "k_corr_gather": 64,
}


def test_output_stage_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, vgprs in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert names, frag
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
