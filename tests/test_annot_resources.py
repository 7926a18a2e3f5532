"""Register / scratch budgets of the annotation kernels (csrc/dbgk_annot.h), read from the built libdbgk.so (no GPU needed).  The
length kernel holds one record and five digit counts; the write kernel one record's five numbers, the composer's 64-bit register
with its three counters, and a number's eight ASCII digits.  64 VGPRs leave every SIMD its eight waves, like the neighbouring output
kernels, and nothing may fall into scratch.

The write kernel does NOT meet 64: it is built with 88 VGPRs.  Its body is straight-line code -- five literals as constant dwords and
five numbers of eight multiply-shift steps each, all unrolled -- and the compiler overlaps the five independent digit chains, which
keeps their 64-bit digit registers and the multiply constants alive together.  Its waves are bounded by LDS before registers: a
workgroup holds 256 x 120 + 32 = 30 752 bytes, so a CU's 160 KiB take five workgroups, five waves per SIMD, and 512 / 5 = 102 VGPRs
(96 at the allocation granule of 8) cost no wave.  Its budget is therefore 96, the most that keeps the LDS-bound occupancy, not 64.

The counts are exact: one length kernel, one write kernel, one check kernel, no
template forms.  The kernels carry none of the name fragments the other stages' resource tests count (k_fmt_, k_emit_, k_pair_,
k_parse_, k_gz_, and the five k_corr_ kernel names)."""
from test_kernel_resources import kernel_metadata  # noqa: F401  (same reader as the hot kernels' budget test)

BUDGETS = {   # kernel name fragment -> (max VGPRs, instances)
    "k_annot_len": (64, 1),
    "k_annot_write": (96, 1),   # built: 88 (the docstring says why 64 is not met and what 96 keeps)
    "k_annot_check": (64, 1),
}


def test_annotation_kernels_fit(tmp_path):
    meta = kernel_metadata(tmp_path)
    found = [n for n in meta if "k_annot_" in n and not n.endswith(".kd")]
    assert len(found) == 3, found
    for n in found:
        # (the argument type dbgk_corr_rec is part of the mangled names; the corrector's test counts its kernels by their full names)
        assert not any(frag in n for frag in ("k_fmt_", "k_emit_", "k_pair_", "k_parse_", "k_gz_", "k_corr_classify", "k_corr_fix", "k_corr_overflow",
                                              "k_corr_seal", "k_corr_from_counts")), n
    for frag, (vgprs, instances) in BUDGETS.items():
        names = [n for n in found if frag in n]
        assert len(names) == instances, (frag, names)
        for n in names:
            m = meta[n]
            print(n, m)
            assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
            assert m["vgpr_count"] + m.get("agpr_count", 0) <= vgprs, (n, m)
            assert m.get("max_flat_workgroup_size", 256) == 256, (n, m)
