"""Register / scratch budgets of the cleaner's output-stage kernels, read from the built libdbgk.so (no GPU needed).
The gather keeps nothing in LDS but its two search results; a lane holds two 16-byte vectors, a read's three offsets and the
two source dwords of the word it composes, the length kernel its seven 64-bit counters: 64 VGPRs leave every SIMD its eight
waves, and nothing may fall into scratch.  Both record types of the length kernel and all three forms of the gather (bases
alone, two planes, two planes with the N substitution) are held to it."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, instances)
    "k_clean_out_len": (64, 2),
    "k_clean_gather": (64, 3),
}


def test_output_stage_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, (vgprs, instances) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == instances, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
