"""Register / scratch budgets of the correct_error_reads kernels, read from the built libdbgk.so (no GPU needed).
The tree frontier and the read live in LDS or global memory, indexed by lane; none of it may fall into scratch."""
import pytest

from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> max VGPRs
    "k_corr_classify": 128,
    "k_corr_fix": 128,
    "k_corr_overflow": 128,
    "k_corr_seal": 64,
    "k_corr_from_counts": 64,
}


def test_correct_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, vgprs in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert names, frag
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] <= vgprs, (n, m)
