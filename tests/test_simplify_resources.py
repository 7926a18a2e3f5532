"""Register / scratch budgets of the kernels that trace the simplification paths, read from the built libdbgk.so (no GPU needed).
They are chains of dependent probes -- one walk per thread, latency hidden by occupancy alone -- so none may use scratch and every
budget stays at or below the 64 VGPRs that still give eight waves per SIMD.  Below that each kernel gets what its own state needs
plus some room, so that a kernel that starts to keep more in registers is noticed."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> max VGPRs
    # the walk's state: slot, direction, length, depth sum, cutoff; per step one 16-byte node, the neighbour's key and its reverse
    # complement, hash, probe slot and probe counter as 64-bit values, and the table's fields (what the successor kernel of the read-out keeps, in a loop)
    "k_simp_trace": 40,
    "k_simp_branches": 40,     # the same walk behind one more neighbour step; the row lives in registers until it is stored
    "k_simp_fill": 40,         # the same walk and the two output pointers
    # 128-bit keys: the key, its neighbour and the reverse complement are two words each, the comparison and the match test too
    "k_wsimp_trace": 48,
    "k_wsimp_branches": 48,
    "k_wsimp_fill": 48,
    "k_simp_update": 16,       # an index, a slot, the 8-byte link pair, a record, a flag byte and five base pointers
}


def test_simplify_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, vgprs in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == 1, (frag, names)
        m = meta[names[0]]
        print(names[0], m["vgpr_count"], m.get("agpr_count", 0), m.get("private_segment_fixed_size", 0))
        assert m.get("private_segment_fixed_size", 0) == 0, (names[0], m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (names[0], m)
    assert len([n for n in meta if ("k_simp_" in n or "k_wsimp_" in n) and not n.endswith(".kd")]) == len(BUDGETS)
