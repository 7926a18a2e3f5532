"""Register / scratch budgets of the PAIR stage's kernels (csrc/dbgk_pair.h), read from the built libdbgk.so (no GPU needed).  The
gather is the register gather of the output stage with two source planes per output plane: a lane holds two 16-byte vectors, a
read's offsets, one 64-bit source address per plane and the two source dwords of the word it composes; nothing but the two search
results lies in LDS.  The classify kernel holds two 64-bit and four 32-bit tallies, the scatter kernel a pair's offsets and ranks.
64 VGPRs leave every SIMD its eight waves, like the output stage's kernels, and nothing may fall into scratch.  The counts are
exact: classify, scatter, and the gather with and without quality planes -- there are no others, and the stage adds no form of the
k_emit_ kernels (tests/test_emit_resources.py counts those)."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, instances)
    "k_pair_classify": (64, 1),
    "k_pair_scatter": (64, 1),
    "k_pair_gatherILb": (64, 2),
}


def test_pair_stage_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert len([n for n in meta if "k_pair_" in n and not n.endswith(".kd")]) == 4
    for frag, (vgprs, instances) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == instances, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
