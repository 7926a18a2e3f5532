"""Register / scratch budgets of the output-stage kernels the corrector and the cleaner share (csrc/dbgk_emit.h), read from the
built libdbgk.so (no GPU needed).  The register gather keeps nothing in LDS but its two search results; a lane holds two 16-byte
vectors, a read's three offsets and the two source dwords of the word it composes.  The corrector's one-plane gather keeps a
tile, a list of reads and the two search results in LDS; a lane holds one 16-byte vector and a few offsets.  The length kernel
holds the 64-bit counters of its rule (eleven for the corrector, seven for the cleaner).  64 VGPRs leave every SIMD its eight
waves, and nothing may fall into scratch.  All three rules of the length kernel (the corrector's records, lowqual blocks,
adapter hits), all three forms of the register gather (bases alone, two planes, two planes with the N substitution) and the
one LDS gather are held to it, and the counts are exact: there are no others."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, instances)
    "k_emit_out_len": (64, 3),
    "k_emit_gatherILb": (64, 3),
    "k_emit_gather_lds": (64, 1),
}


def test_output_stage_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert len([n for n in meta if "k_emit_" in n and not n.endswith(".kd")]) == 7
    for frag, (vgprs, instances) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == instances, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
