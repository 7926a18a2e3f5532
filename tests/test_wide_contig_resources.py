"""Register / scratch budgets of the two contig read-out kernels on 128-bit keys, read from the built libdbgk.so (no GPU needed).
Neither may use scratch.  Like their 64-bit counterparts (tests/test_contig_resources.py) they are streaming kernels of 256 threads
whose time goes into dependent loads, so both stay at or below the 64 VGPRs that still give eight waves per SIMD; below that each
gets its counterpart's budget plus what the second key word adds."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> max VGPRs
    "k_wctg_successors": 56,   # k_contig_successors' 40 plus a second 64-bit word for the node's key, the neighbour's key, its reverse complement and the picked key
    "k_wctg_emit": 56,         # k_contig_emit's 48 plus the second word of the anchor's k-mer, its slot, and the shift that picks the word
}


def test_wide_contig_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, vgprs in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == 1, (frag, names)
        m = meta[names[0]]
        assert m.get("private_segment_fixed_size", 0) == 0, (names[0], m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs <= 64, (names[0], m)
        assert "k_contig_" not in names[0]   # the ten k_contig_* kernels stay ten
    assert len([n for n in meta if "k_wctg_" in n and not n.endswith(".kd")]) == len(BUDGETS)
