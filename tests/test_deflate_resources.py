"""Register / scratch budgets of the DEFLATE stage's kernels (csrc/dbgk_gz.h), read from the built libdbgk.so (no GPU needed).  The
count is exact: members, gather.  The member kernel keeps the piece, the tables and every array of the code construction in LDS --
lane 0 derives the codes there, indexing nothing in registers by a variable --, so nothing may fall into scratch; 128 VGPRs would
still give four waves per SIMD of 512 registers, though its 70 KiB of LDS admit two workgroups per compute unit.  Both kernels are
launched with 256 threads."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, instances)
    "k_gz_members": (128, 1),
    "k_gz_gather": (128, 1),
}


def test_deflate_stage_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert len([n for n in meta if "k_gz_" in n and not n.endswith(".kd")]) == 2
    for frag, (vgprs, instances) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == instances, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
