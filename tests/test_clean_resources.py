"""Register / scratch budgets of the clean_adapter / clean_lowqual kernels, read from the built libdbgk.so (no GPU needed).
The alignment keeps running state per diagonal only: no matrix, so nothing of it may fall into scratch."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)


def test_clean_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    names = [n for n in meta if "k_clean_" in n and not n.endswith(".kd")]
    assert len([n for n in names if "k_clean_adapter" in n]) >= 2, names  # the LDS form and the global-memory form
    assert [n for n in names if "k_clean_lowqual" in n], names
    for n in names:
        m = meta[n]
        assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= 128, (n, m)
