"""GPU: the PARSE stage (csrc/dbgk_parse.h) -- the bytes of a FASTQ / FASTA text to the device batch.  Crafted texts
(tests/parse_cases.py) through Parser.chunk against the plain restatement of the rule (tests/parse_restatement.py, anchored to the
host readers by tests/test_parse_cpu.py) byte for byte: whole 16-byte vectors of both planes with the zero pad, offsets, records,
every counter and `consumed`, with last 1 and 0, with and without a quality plane; a text cut at every byte of a record through one
handle; device input inside a larger buffer of newlines and markers; the hand-overs to the cleaner and to a graph handle.  Each GPU
step is a child process under a time limit of its own (tests/parse_gpu_steps.py); the limits only end a stuck step.  Every test here
fails without the stage: capi.Parser does not exist."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parse_cases as PC  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "parse_gpu_steps.py")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_crafted_texts_equal_the_restatement_byte_for_byte():
    res = run_step("crafted", 180)
    print(res)
    names = [k for k, v in PC.cases().items() if v[1].count(b"\n") < 60000]
    assert len(names) > 60 and all(n in res for n in names)
    zero = {"n_records": 0, "n_lines": 0, "ignored_lines": 0, "n_bases": 0, "mismatched": 0}
    assert res["empty"] == zero
    assert res["one_byte"] == res["no_newline_no_marker"] == dict(zero, n_lines=1, ignored_lines=1)
    assert res["one_byte_marker"] == res["header_only"] == res["header_only_newline"] == dict(zero, n_lines=1, n_records=1)
    assert res["one_record"] == res["one_record_no_final_newline"] == dict(zero, n_lines=4, n_records=1, n_bases=5)
    assert res["norecords_fq"]["n_records"] == 0 and res["norecords_fq"]["ignored_lines"] == res["norecords_fq"]["n_lines"] > 0
    assert res["quality_starts_with_at"] == dict(zero, n_lines=12, n_records=3, n_bases=8)
    assert res["separator_starts_with_at"] == dict(zero, n_lines=8, n_records=2, n_bases=7)
    assert res["crlf"]["n_bases"] == 5 + 3   # the '\r' stays with its line
    assert res["fasta_junk_and_sequence_with_marker"] == dict(zero, n_lines=10, n_records=3, ignored_lines=4, n_bases=7)
    for n in (63, 64, 65, 255, 256, 257):
        for junk in (0, 1, 2, 3):   # every line has the marker: records at lines junk, junk + 4, ...
            assert res["all_marker_fastq_%d_lines_behind_%d" % (n, junk)] == dict(zero, n_lines=n + junk, ignored_lines=junk, n_records=(n + 3) // 4,
                                                                                   n_bases=6 * ((n + 2) // 4))
        for junk in (0, 1):
            assert res["all_marker_fasta_%d_lines_behind_%d" % (n, junk)]["n_records"] == (n + 1) // 2
    assert res["lengths_0_100_residues"] == "all"


@pytest.mark.gpu
def test_the_map_scan_crosses_many_workgroups_and_rounds_of_the_spine():
    res = run_step("many", 240)
    print(res)
    for junk in (0, 1, 2, 3):
        assert res["all_marker_fastq_70001_lines_behind_%d" % junk]["n_records"] == 70004 // 4
    n = 256 * PC.CHUNK + 3 * PC.CHUNK + 5
    assert res["all_marker_fastq_%d_short_lines_behind_1" % n]["n_records"] == (n + 3) // 4


@pytest.mark.gpu
def test_a_text_cut_at_every_byte_of_a_record_gives_the_batch_of_the_whole_text():
    res = run_step("chunking", 180)
    print(res)
    assert 30 < res["cuts"] <= 100 and res["consumed_0"] >= 1 and res["consumed_0_in_stream_of_3"] == 0


@pytest.mark.gpu
def test_device_input_is_read_in_place_and_nothing_outside_it_counts():
    res = run_step("device_input", 120)
    print(res)
    assert len(res) == 4 and all(v["n_records"] > 0 for v in res.values())


@pytest.mark.gpu
def test_the_parsed_batch_through_clean_lowqual_equals_the_reference_files():
    res = run_step("lowqual", 180)
    print(res)
    assert sorted(res) == ["lowqual_default", "lowqual_e01", "lowqual_mixed_plain"]
    assert res["lowqual_mixed_plain"]["mismatched"] == res["lowqual_e01"]["mismatched"] == 1 and res["lowqual_default"]["mismatched"] == 0


@pytest.mark.gpu
def test_the_parsed_batch_pushed_into_a_graph_equals_the_same_reads_from_the_host():
    res = run_step("graph", 300)
    print(res)
    assert res["direct"] == res["partition"] and res["direct"]["reads"] == 3000 and res["direct"]["nodes"] > 1000


@pytest.mark.gpu
def test_the_error_returns():
    from dbg_assembly_amd import capi
    res = run_step("states", 120)
    print(res)
    want = {"with_quals_for_fasta": capi.ERR_ARG, "format_3": capi.ERR_ARG, "results_before_a_chunk": capi.ERR_STATE,
            "device_before_a_chunk": capi.ERR_STATE, "push_before_a_chunk": capi.ERR_STATE, "n_bytes_2_to_the_31": capi.ERR_ARG,
            "n_bytes_2_to_the_31_device": capi.ERR_ARG, "misaligned_text": capi.ERR_ARG, "results_after_a_refused_chunk": capi.ERR_STATE,
            "empty_chunk": capi.OK, "empty_chunk_device": capi.OK, "own_bases_as_input": capi.ERR_ARG, "own_quals_as_input": capi.ERR_ARG,
            "results_after_refused_input": capi.OK, "quality_plane_of_a_batch_without_one": capi.ERR_ARG, "results_with_no_pointer": capi.OK,
            "push_into_a_finalized_handle": capi.ERR_STATE}
    assert res == want
