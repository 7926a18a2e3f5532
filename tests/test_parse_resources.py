"""Register / scratch budgets of the PARSE stage's kernels (csrc/dbgk_parse.h), read from the built libdbgk.so (no GPU needed).  The
two line kernels hold one 16-byte vector of text, its 16 newline bits and a running count; the three map kernels one composed
map per thread plus the few bytes of the eight lines they step through; the record kernel one dbgk_parse_rec.  LDS holds four
words per workgroup (wave totals or wave maps) and the record kernel's one counter.  64 VGPRs leave every SIMD its eight waves, like
the output stage's kernels, and nothing may fall into scratch -- the newline bits in particular are taken out of the vector without
indexing it by a variable.  The count is exact: count, lines, map_reduce, map_spine, states, records.  The gather is the output
stage's k_emit_gather<false, false>, once per plane; the stage adds no form of the k_emit_ or k_pair_ kernels
(tests/test_emit_resources.py and tests/test_pair_resources.py count those)."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, instances)
    "k_parse_count": (64, 1),
    "k_parse_lines": (64, 1),
    "k_parse_map_reduce": (64, 1),
    "k_parse_map_spine": (64, 1),
    "k_parse_states": (64, 1),
    "k_parse_records": (64, 1),
}


def test_parse_stage_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert len([n for n in meta if "k_parse_" in n and not n.endswith(".kd")]) == 6
    for frag, (vgprs, instances) in BUDGETS.items():
        names = [n for n in meta if frag in n and not n.endswith(".kd")]
        assert len(names) == instances, (frag, names)
        for n in names:
            m = meta[n]
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
