"""GPU: the FORMAT stage (csrc/dbgk_format.h) -- a compact batch, its headers in the parsed text and the host's suffixes to the
bytes of a FASTQ / FASTA file.  Crafted batches (tests/format_cases.py) through Formatter.format against the plain restatement of
the rule (tests/format_restatement.py, anchored to the host writer and the reference's files by tests/test_format_cpu.py) byte for
byte: the whole 16-byte vectors with the zero pad, results() and every counter; device input inside larger buffers of newlines and
markers; the chain Parser -> Cleaner -> Formatter -> Parser / Deflater on the CLEAN goldens; every error return.  Each GPU step is a
child process under a time limit of its own (tests/format_gpu_steps.py); the limits only end a stuck step.  Every test here fails
without the stage: capi.Formatter does not exist."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import format_cases as FC  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "format_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_crafted_batches_equal_the_restatement_byte_for_byte():
    res = run_step("crafted", 180)
    print(res)
    cases = FC.cases()
    assert len(cases) > 40 and all(n in res for n in cases)
    zero = {"n_records": 0, "out_bytes": 0, "head_bytes": 0, "suffix_bytes": 0, "seq_bytes": 0}
    assert res["empty_fastq"] == res["empty_fasta"] == zero
    assert res["minimal_fastq"] == dict(zero, n_records=1, out_bytes=6, head_bytes=1)
    assert res["minimal_fasta"] == dict(zero, n_records=1, out_bytes=3, head_bytes=1)
    assert res["no_bytes_at_all_fastq"] == dict(zero, n_records=2, out_bytes=10)
    assert res["no_bytes_at_all_fasta"] == dict(zero, n_records=2, out_bytes=4)
    assert res["fasta_5000_records_of_3_bytes"] == dict(zero, n_records=5000, out_bytes=15000, head_bytes=5000)
    for tag, per in (("fastq", 2), ("fasta", 1)):
        s = res["sweep_0_100_" + tag]
        assert s["head_bytes"] == s["suffix_bytes"] == s["seq_bytes"] == 3 * 5050
        assert s["out_bytes"] == (2 + per) * 3 * 5050 + 303 * (5 if tag == "fastq" else 2)
        assert res["run_of_3T_emptied_records_" + tag]["n_records"] == 3 * FC.T + 2
        assert res["pieces_of_3T_and_100_" + tag]["suffix_bytes"] == 2 + 2 * ((3 * FC.T + 100) // 2)
        for extra in (0, 1):
            assert res["output_of_16384%+d_bytes_%s" % (extra, tag)]["out_bytes"] == 16384 + extra
        for d in (-1, 0, 1, 2):
            assert res["first_record_ends_at_T%+d_%s" % (d, tag)]["n_records"] == 2
    assert res["marker_3e_fastq"] == res["marker_40_fastq"]
    assert res["handles"] == 6   # FASTQ and FASTA with the markers 0, '>' and '@', each handle used for many batches in a row
    assert list(cases)[-1] == "small_after_large_fastq" and res["small_after_large_fastq"]["out_bytes"] == 22


@pytest.mark.gpu
def test_device_input_is_read_in_place_and_nothing_outside_it_counts():
    res = run_step("device_input", 120)
    print(res)
    assert len(res) == 7 and sum(v["n_records"] > 0 for v in res.values()) == 6


@pytest.mark.gpu
def test_parse_clean_format_gives_the_reference_files_and_parses_and_deflates_in_place():
    res = run_step("chain", 180)
    print(res)
    assert sorted(v["input"] for v in res.values()) == ["mixed.fq", "phred64.fq", "reads.fq"]
    assert all(v["records"] > 0 and v["out_bytes"] > 0 for v in res.values())
    assert [v["mismatched"] for v in res.values() if v["input"] == "mixed.fq"] == [1]


@pytest.mark.gpu
def test_the_error_returns():
    from dbg_assembly_amd import capi
    res = run_step("states", 120)
    print(res)
    arg = ("format_3", "marker_256", "fastq_without_a_quality_plane", "fasta_with_a_quality_plane", "fastq_without_a_quality_plane_device",
           "fasta_with_a_quality_plane_device", "misaligned_text", "misaligned_bases", "misaligned_quals", "n_text_2_to_the_31", "n_2_to_the_31",
           "own_output_as_text", "own_output_as_bases", "own_output_as_quals", "header_leaves_the_text", "decreasing_offsets_device",
           "decreasing_offsets_host", "decreasing_suffix_offsets", "suffix_offsets_from_1", "capacity_below_the_text")
    state = ("results_before_a_call", "device_before_a_call", "recs_of_a_parser_before_a_chunk", "text_of_a_parser_before_a_chunk", "results_after_refused_calls",
             "results_after_a_header_that_leaves_the_text", "results_after_decreasing_offsets")
    ok = ("good_call", "results_after_refused_input", "header_ends_with_the_text", "no_records", "fasta_good_call", "recs_of_a_parser_after_a_chunk",
          "text_of_a_parser_after_a_chunk")
    want = dict([(k, capi.ERR_ARG) for k in arg] + [(k, capi.ERR_STATE) for k in state] + [(k, capi.OK) for k in ok])
    assert res == want


def clean_cases():
    import clean_restatement as CR
    return CR.golden_cases(FC.CLEAN)


@pytest.mark.gpu
@pytest.mark.parametrize("case", clean_cases(), ids=lambda c: c["name"])
def test_the_programs_run_file_to_file_on_the_device(tmp_path, case):
    """bin/clean_lowqual and bin/clean_adapter with DBGK_TEXT=device, writing through zlib and through the device deflater, two cases
    again with windows that end inside records: the inflated output and the .stat file are the reference's.  bin/clean_adapter
    refuses an input with a quality line that is not as long as its read (mixed.fq holds one) and names the switch."""
    import gzip
    import clean_restatement as CR
    exe = os.path.join(ROOT, "dbg_assembly_amd", "bin", case["program"])
    refused = case["program"] == "clean_adapter" and case["input"].startswith("mixed")
    runs = [{}, {"DBGK_GZ": "device"}]
    if case["name"] in ("lowqual_mixed_plain", "adapter_default"):
        runs += [{"DBGK_TEST_HOOKS": "text_window=1000"}, {"DBGK_GZ": "device", "DBGK_TEST_HOOKS": "text_window=257"}]
    want = CR.expected_outputs(FC.CLEAN, case)
    base = {k: v for k, v in os.environ.items() if k not in ("DBGK_GZ", "DBGK_GUNZIP", "DBGK_TEST_HOOKS")}
    for i, extra in enumerate(runs):
        out, stat = tmp_path / ("out%d.gz" % i), tmp_path / ("out%d.stat" % i)
        r = subprocess.run([exe] + case["args"] + [case["input"], str(out), str(stat)], cwd=FC.CLEAN, capture_output=True, text=True, timeout=120,
                           env=dict(base, DBGK_TEXT="device", **extra))
        if refused:
            assert r.returncode == 1 and "DBGK_TEXT=device" in r.stderr, (extra, r.returncode, r.stderr[-2000:])
            continue
        assert r.returncode == 0, (extra, r.stderr[-3000:])
        assert gzip.decompress(out.read_bytes()).decode("latin-1") == want["out"], extra
        assert stat.read_bytes().decode("latin-1") == want["stat"], extra
        if "DBGK_TEST_HOOKS" in extra:
            assert r.stderr.count("reading num") > 3, extra   # the windows did end inside the file
