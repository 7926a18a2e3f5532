"""Register / scratch budgets of the contig read-out kernels, read from the built libdbgk.so (no GPU needed).  None of them may use
scratch.  All are streaming kernels of 256 threads over slots, ports, nodes or output words whose time goes into dependent loads, so
every budget stays at or below the 64 VGPRs that still give eight waves per SIMD; below that each kernel gets what its own state
needs plus some room, so that a kernel that starts to keep more in registers is noticed."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> max VGPRs
    "k_contig_count_linear": 16,     # a slot index, three flag loads, a counter
    "k_contig_compact_linear": 48,   # the same, a block scan, and the loop over eight sub-tiles unrolled
    "k_contig_successors": 40,       # one 16-byte node, the neighbour's key and its reverse complement, hash and probe slot: 64-bit values
    "k_contig_mutual": 16,           # two port indices and two loads
    "k_contig_rank_init": 16,        # one 16-byte port state
    "k_contig_jump": 16,             # two 16-byte port states
    "k_contig_classify": 24,         # two port states and the two tile sums (one of them 64-bit)
    "k_contig_place": 64,            # two block scans (one 64-bit), two port states and a 48-byte record, loop unrolled
    "k_contig_scatter": 40,          # three port states (the node's two, the anchor's) and the record fields of the side's end
    "k_contig_emit": 48,             # two 8-byte output words, the bisection, and the current contig's offsets, k-mer and record fields
}


def test_contig_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    for frag, vgprs in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == 1, (frag, names)
        m = meta[names[0]]
        assert m.get("private_segment_fixed_size", 0) == 0, (names[0], m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (names[0], m)
    assert len([n for n in meta if "k_contig_" in n and not n.endswith(".kd")]) == len(BUDGETS)
