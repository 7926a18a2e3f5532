"""Register / scratch budgets of the FORMAT stage's kernels (csrc/dbgk_format.h), read from the built libdbgk.so (no GPU needed).  The
length kernel holds one record's six numbers and four running sums; the gather one record as two 64-bit output offsets, three
source addresses and three cumulative lengths, plus the four dwords of its vector.  64 VGPRs leave every SIMD its eight waves, like
the output stage's kernels, and nothing may fall into scratch.  The count is exact: len, and the gather in its two forms (FASTQ,
FASTA).  The stage adds no form of the k_emit_, k_parse_ or k_pair_ kernels (their resource tests count those)."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, instances)
    "k_fmt_len": (64, 1),
    "k_fmt_gather": (64, 2),
}


def test_format_stage_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert len([n for n in meta if "k_fmt_" in n and not n.endswith(".kd")]) == 3
    for frag, (vgprs, instances) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == instances, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
