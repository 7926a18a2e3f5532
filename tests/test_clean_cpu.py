"""CPU: clean_adapter / clean_lowqual -- the command lines, the argument checks of the C ABI, the binding, and the Python
restatement of the two programs against every golden the real reference wrote (tests/golden/clean_*)."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_restatement as CR  # noqa: E402

BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLDEN, "clean_cases")
USAGE = {"clean_adapter": "clean_usage_adapter.txt", "clean_lowqual": "clean_usage_lowqual.txt"}


def golden_cases():
    return CR.golden_cases(CASES)


@pytest.mark.parametrize("prog", sorted(USAGE))
def test_cli_prints_the_reference_usage(prog):
    want = open(os.path.join(GOLDEN, USAGE[prog]), "rb").read()
    for args in ([], ["-h"], ["in.fq", "out.gz"]):   # no arguments, -h, fewer than three files
        r = subprocess.run([os.path.join(BIN, prog)] + args, capture_output=True, timeout=60)
        assert r.returncode == 0 and r.stdout == want, args


def test_cli_refuses_what_the_reference_cannot_do(tmp_path):
    """-s below 1 makes the reference report coordinates it never set; a missing contaminant file ends it with status 255"""
    fq = os.path.join(CASES, "reads.fq")
    r = subprocess.run([os.path.join(BIN, "clean_adapter"), "-a", os.path.join(CASES, "illumina_NEB_adapter.fa"), "-s", "0", fq,
                        str(tmp_path / "o.gz"), str(tmp_path / "o.stat")], capture_output=True, text=True, timeout=60)
    assert r.returncode not in (0, 255) and "-s" in r.stderr and not (tmp_path / "o.gz").exists()
    r = subprocess.run([os.path.join(BIN, "clean_adapter"), "-a", str(tmp_path / "missing.fa"), fq, str(tmp_path / "o.gz"),
                        str(tmp_path / "o.stat")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "fail to open input file: %s" % (tmp_path / "missing.fa") in r.stderr
    # the three default names resolve inside DBGK_ADAPTER_DIR
    r = subprocess.run([os.path.join(BIN, "clean_adapter"), "-a", "R2-adapter", fq, str(tmp_path / "o.gz"), str(tmp_path / "o.stat")],
                       capture_output=True, text=True, timeout=60, env=dict(os.environ, DBGK_ADAPTER_DIR=CASES))
    assert "Used illumina adapter: R2 :   GATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT" in r.stderr


def test_clean_entry_points_validate_before_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.dbgk_clean_create(0, None) == capi.ERR_ARG
    assert L.dbgk_clean_create(-1, ctypes.byref(h)) == capi.ERR_ARG
    off = (ctypes.c_uint64 * 2)(0, 4)
    out = (ctypes.c_int32 * 16)()
    assert L.dbgk_clean_set_adapters(None, b"ACGT", off, 1, 12) == capi.ERR_ARG
    assert L.dbgk_clean_adapter(None, b"ACGT", off, 1, out) == capi.ERR_ARG
    assert L.dbgk_clean_lowqual(None, b"ACGT", b"IIII", off, 1, 0.001, 33, out) == capi.ERR_ARG
    assert L.dbgk_clean_batch_stats(None, None) == capi.ERR_ARG
    assert L.dbgk_clean_destroy(None) == capi.ERR_ARG


def test_binding_covers_the_clean_section():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in ("dbgk_clean_create", "dbgk_clean_destroy", "dbgk_clean_set_adapters", "dbgk_clean_adapter", "dbgk_clean_lowqual",
              "dbgk_clean_batch_stats"):
        assert n in names and hasattr(capi.lib(), n)
    assert capi.ADAPTER_HIT_DTYPE.itemsize == 24 and capi.LOWQUAL_BLOCK_DTYPE.itemsize == 24
    assert capi.LOWQUAL_BLOCK_DTYPE.fields["start"][1] == 8 and ctypes.sizeof(capi.CleanStats) == 8 * 8
    assert capi.lib().dbgk_abi_version() == 7
    assert hasattr(capi.Cleaner, "__enter__") and hasattr(capi.Cleaner, "__exit__")


def test_no_cleaner_without_gpu(tmp_path):
    """no device: the binding raises and the programs exit non-zero with a message, nothing falls back to the host"""
    from dbg_assembly_amd import capi
    if capi.lib().dbgk_device_count() > 0:
        return
    with pytest.raises(capi.DbgkError) as e:
        capi.Cleaner()
    assert e.value.status == capi.ERR_HIP
    for prog, args in (("clean_adapter", ["-a", "illumina_NEB_adapter.fa"]), ("clean_lowqual", [])):
        r = subprocess.run([os.path.join(BIN, prog)] + args + ["reads.fq", str(tmp_path / "o.gz"), str(tmp_path / "o.stat")], cwd=CASES,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "dbgk_clean_create failed" in r.stderr


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_golden(case):
    want = CR.expected_outputs(CASES, case)
    got = CR.run_case(CASES, case)
    assert got["out"] == want["out"]
    assert got["stat"] == want["stat"]


def test_three_formulations_of_the_alignment_agree():
    """per diagonal (what the kernel does), the reference's matrix, and the numpy form the large GPU job is checked with"""
    for case in golden_cases():
        if case["program"] != "clean_adapter" or "norecords" in case["name"]:
            continue
        o = CR.case_options(case)
        adapters = CR.case_adapters(CASES, case)
        reads = [s for _, s, _ in CR.load_reads(os.path.join(CASES, case["input"]))]
        many = CR.align_many([s.encode("latin-1") for s in reads], adapters, o["-s"], cells_per_chunk=20000)
        for s, m in zip(reads, many):
            assert CR.first_hit(s, adapters, o["-s"]) == m, (case["name"], s[:40])
            if len(s) <= 200:
                for _, ad in adapters:
                    assert CR.align(s, ad) == CR.align_matrix(s, ad)
    assert CR.align("ACNAC", "ACNAC") == (2, 1, 2, 1, 2)            # N against N is -2: the run ends, and the first of two equal runs wins
    assert CR.align("ACGTNACGT", "ACGTNACGT") == (6, 1, 9, 1, 9)    # 4 - 2 + 4: the run survives one mismatch
    assert CR.align("", "ACGT") == (0, 0, 0, 0, 0)


def test_goldens_cover_what_they_are_meant_to():
    """every category the issue lists shows in each adapter case; the inputs hold the record shapes it names"""
    cases = {c["name"]: c for c in golden_cases()}
    for name in ("adapter_default", "adapter_contaminants", "adapter_mixed_plain"):
        seen = CR.adapter_coverage(CASES, cases[name])
        assert not [n for n in CR.NEED_ADAPTER if n not in seen], name
    recs = CR.load_reads(os.path.join(CASES, "mixed.fq"))
    assert recs == CR.load_reads(os.path.join(CASES, "mixed.fq.gz"))
    lens = [len(s) for _, s, _ in recs]
    assert min(lens) == 0 and 30 in lens and max(lens) == 2000
    assert any(len(s) != len(q) for _, s, q in recs) and any(s and s == s.lower() for _, s, _ in recs) and any("N" in s for _, s, _ in recs)
    assert len(recs) * 4 < open(os.path.join(CASES, "mixed.fq")).read().count("\n")    # lines that belong to no record
    contam = CR.read_fasta(open(os.path.join(CASES, "contaminants.fa")).read(), 1)
    assert [len(s) for _, s in contam] == [130, 130, 8, 8] and "N" in contam[0][1] and contam[1][0] == "long130 minus-strand"
    assert CR.load_reads(os.path.join(CASES, "norecords.fq")) == []
    for name in ("adapter_norecords", "lowqual_norecords"):
        assert "-nan" in CR.expected_outputs(CASES, cases[name])["stat"]
    texts = "".join(CR.expected_outputs(CASES, c)["out"] for c in golden_cases() if c["program"] == "clean_lowqual")
    assert "TrimLowQual" in texts and "FilterShort" in texts and "RQ: -nan%" in texts
