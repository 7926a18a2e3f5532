"""GPU: the annotation of the corrector's headers composed on the device (csrc/dbgk_annot.h), the formatter reading a suffix plane
where it lies, and bin/correct_error_reads / bin/kmerfreq file to file with DBGK_TEXT=device.  Crafted records
(tests/annot_cases.py) through compact_from + annotate against the plain restatement (tests/annot_restatement.py, anchored to the
reference's files by tests/test_annot_cpu.py) byte for byte, the zero pad included; the suffixed cases of tests/format_cases.py with
the plane uploaded by the test; every error return; the chain Parser -> Corrector -> compact -> annotate -> Formatter -> Parser /
Deflater on the corrector's goldens; the programs against the goldens and against their own host route.  Each GPU step is a child
process under a time limit of its own (tests/annot_gpu_steps.py); the limits only end a stuck step.  Every test here fails without
the feature: the bindings do not exist, and the programs print no `Text on device:` line.

The program cases are those with a table file in the repository: correct_k12, and the 22 of the 25 correct_edges scenarios of
k <= 13 (the tables of k = 15, 16, 17 are built in memory by their own tests and have no file a program could load)."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import annot_cases as AC  # noqa: E402
import format_cases as FC  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "annot_gpu_steps.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
SWITCHES = ("DBGK_TEXT", "DBGK_GZ", "DBGK_GUNZIP", "DBGK_TEST_HOOKS", "DBGK_TIMINGS", "DBGK_GPUS", "DBGK_GPU_LIST")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_crafted_records_equal_the_restatement_byte_for_byte():
    res = run_step("crafted", 180)
    print(res)
    cases = AC.cases()
    assert list(res) == list(cases)
    for name, c in cases.items():
        assert res[name] == {"n": len(c["rec"]), "suffix_bytes": int(AC.expected(c)[1][-1])}, name
    assert res["n_0"] == {"n": 0, "suffix_bytes": 0}
    assert res["all_minimal"]["suffix_bytes"] == 1000 * AC.MIN_SUFFIX
    assert res["all_maximal"]["suffix_bytes"] == (2 * AC.GROUP + 88) * 111
    assert [res["suffix_bytes_16384%+d" % e]["suffix_bytes"] for e in (0, 1)] == [16384, 16385]


@pytest.mark.gpu
def test_the_formatter_reads_a_device_plane_as_it_reads_the_host_s():
    import annot_gpu_steps as S
    res = run_step("formatter", 180)
    print(res)
    cases = S.suffix_cases()
    assert len(cases) > 10 and sorted(res) == sorted(cases)
    assert all(v["suffix_bytes"] > 0 for v in res.values())
    assert {c["fmt"] for c in cases.values()} == {FC.FASTQ, FC.FASTA}


@pytest.mark.gpu
def test_the_error_returns():
    from dbg_assembly_amd import capi
    res = run_step("states", 120)
    print(res)
    arg = ("offsets_from_1", "decreasing_offsets", "total_of_2_to_the_32", "total_of_2_to_the_32_less_1_without_a_plane", "misaligned_plane",
           "misaligned_offsets", "own_output_as_plane")
    state = ("annot_before_a_compact_batch", "annot_device_before_a_compact_batch", "annot_device_before_annot", "annot_results_before_annot",
             "annot_device_after_the_next_compact", "results_before_a_call", "results_after_offsets_from_1", "results_after_decreasing_offsets",
             "results_after_a_total_of_2_to_the_32")
    ok = ("annot", "annot_device_after_annot", "good_call", "good_call_again", "good_call_once_more", "results_after_refused_arguments", "no_plane_at_all",
          "all_empty_suffixes")
    want = dict([(k, capi.ERR_ARG) for k in arg] + [(k, capi.ERR_STATE) for k in state] + [(k, capi.OK) for k in ok])
    assert res == want


@pytest.mark.gpu
def test_parse_correct_annotate_format_gives_the_reference_files_and_parses_and_deflates_in_place():
    import annot_gpu_steps as S
    res = run_step("chain", 300)
    print(res)
    assert sorted(res) == sorted(b[0] for b in S.golden_batches()) and len(res) >= 25
    assert all(v["records"] > 0 and v["suffix_bytes"] >= AC.MIN_SUFFIX * v["records"] for v in res.values())


# ---- the programs ------------------------------------------------------------------------------------------------------------------

def program_cases():
    out = [("correct_k12", c) for c in json.load(open(os.path.join(GOLDEN, "correct_k12", "cases.json")))]
    out += [("correct_edges", c) for c in json.load(open(os.path.join(GOLDEN, "correct_edges", "cases.json"))) if c["table"]]
    return out


def base_env():
    return {k: v for k, v in os.environ.items() if k not in SWITCHES}


def without_run_time(stderr):
    return [line for line in stderr.splitlines() if not line.startswith("Run time:")]


def run_corrector(args, table, lib, **env):
    r = subprocess.run([os.path.join(BIN, "correct_error_reads")] + args + [table, str(lib)], capture_output=True, text=True, timeout=120,
                       env=dict(base_env(), **env))
    assert r.returncode == 0, (env, r.stderr[-3000:])
    return r.stderr


def windows_of(stderr):
    lines = [line for line in stderr.splitlines() if line.startswith("Text on device: ")]
    assert len(lines) == 1, stderr[-2000:]
    return int(lines[0].split()[3])


@pytest.mark.gpu
@pytest.mark.parametrize("d,case", program_cases(), ids=lambda v: v if isinstance(v, str) else v["name"])
def test_correct_error_reads_runs_file_to_file_on_the_device(tmp_path, d, case):
    """the inflated output and the .stat file are the goldens'; stderr is the host route's; DBGK_TIMINGS shows the route"""
    D = os.path.join(GOLDEN, d)
    reads = tmp_path / case["reads"]
    shutil.copy(os.path.join(D, case["reads"]), reads)
    lib = tmp_path / "reads.lib"
    lib.write_text("%s\n" % reads)
    table = os.path.join(D, case.get("table", "table.cz"))
    want_fa = gzip.open(os.path.join(D, case["name"] + ".correct.fa.gz"), "rb").read()
    want_stat = open(os.path.join(D, case["name"] + ".correct.stat"), "rb").read()
    out, stat = str(reads) + ".correct.fa.gz", str(reads) + ".correct.stat"

    def check(extra):
        assert gzip.open(out, "rb").read() == want_fa, extra
        assert open(stat, "rb").read() == want_stat, extra
        os.remove(out)
        os.remove(stat)
    host = run_corrector(case["args"], table, lib)
    assert "Text on device" not in host
    check("host")
    assert without_run_time(run_corrector(case["args"], table, lib, DBGK_TEXT="device")) == without_run_time(host)
    check("DBGK_TEXT=device")
    timed = run_corrector(case["args"], table, lib, DBGK_TEXT="device", DBGK_GZ="device", DBGK_TIMINGS="1")
    assert windows_of(timed) == 1
    assert open(out, "rb").read()[:4] == b"\x1f\x8b\x08\x04"   # BGZF members: the device deflater wrote the file
    check("DBGK_GZ=device")
    if case["name"] in ("default", "mask_words"):
        for window in (257, 1000):
            hooked = run_corrector(case["args"], table, lib, DBGK_TEXT="device", DBGK_TIMINGS="1", DBGK_TEST_HOOKS="text_window=%d" % window)
            assert windows_of(hooked) > 3
            check("text_window=%d" % window)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["crlf", "last_record_lacks_its_sequence_line"])
def test_odd_line_ends_go_the_way_of_the_host_route(tmp_path, shape):
    D = os.path.join(GOLDEN, "correct_k12")
    case = json.load(open(os.path.join(D, "cases.json")))[0]
    lines = gzip.open(os.path.join(D, case["reads"]), "rb").read().split(b"\n")[:4 * 150]
    if shape == "crlf":
        text = b"".join(line + b"\r\n" for line in lines)
    else:
        text = b"".join(line + b"\n" for line in lines) + b"@the_last_one no sequence line follows"
    reads = tmp_path / "reads.fq"
    reads.write_bytes(text)
    lib = tmp_path / "reads.lib"
    lib.write_text("%s\n" % reads)
    got = {}
    for route, env in (("host", {}), ("device", {"DBGK_TEXT": "device"})):
        stderr = run_corrector(case["args"], os.path.join(D, "table.cz"), lib, **env)
        got[route] = (gzip.open(str(reads) + ".correct.fa.gz", "rb").read(), open(str(reads) + ".correct.stat", "rb").read(), without_run_time(stderr))
        os.remove(str(reads) + ".correct.fa.gz")
    assert got["device"] == got["host"]
    assert got["host"][0].count(b"\n") == 2 * (150 + (shape != "crlf")) and (b"\r" in got["host"][0]) == (shape == "crlf")


@pytest.mark.gpu
def test_j1_under_the_switch_still_writes_the_reference_s_merged_files(tmp_path):
    import pair_restatement as PR
    from pair_gpu_steps import golden, rotated_fq
    meta = {c["name"]: c for c in json.load(open(os.path.join(PR.CORRECT, "cases.json")))}
    f1, f2 = str(tmp_path / "reads_1.fq.gz"), str(tmp_path / "reads_2.fq")
    shutil.copy(os.path.join(PR.CORRECT, "reads.fq.gz"), f1)
    rotated_fq(f1, f2)
    lib = tmp_path / "reads.lib"
    lib.write_text("%s\n%s\n" % (f1, f2))
    stderr = run_corrector(meta["default"]["args"] + ["-j", "1"], os.path.join(PR.CORRECT, "table.cz"), lib, DBGK_TEXT="device", DBGK_TIMINGS="1")
    assert stderr.count("Text on device: ") == 2 and "Merge all the paired reads files completed" in stderr
    pair, single, stat = golden("default")
    assert gzip.open(f1 + ".correct.fa.gz.pair.fa.gz", "rb").read() == pair
    assert gzip.open(f1 + ".correct.fa.gz.single.fa.gz", "rb").read() == single
    assert open(f1 + ".correct.fa.gz.pair.single.stat", "rb").read() == stat


@pytest.mark.gpu
def test_kmerfreq_counts_the_same_tables_from_text_parsed_on_the_device(tmp_path):
    reads = os.path.join(GOLDEN, "correct_k12", "reads.fq.gz")
    lib = tmp_path / "reads.lib"
    lib.write_text("%s\n" % reads)
    files = {}
    for route, env in (("host", {}), ("device", {"DBGK_TEXT": "device"}), ("windows", {"DBGK_TEXT": "device", "DBGK_TEST_HOOKS": "text_window=1000"})):
        prefix = tmp_path / route
        r = subprocess.run([os.path.join(BIN, "kmerfreq"), "-k", "12", "-f", "1", "-o", str(prefix), str(lib)], capture_output=True, text=True, timeout=120,
                           env=dict(base_env(), DBGK_TIMINGS="1", **env))
        assert r.returncode == 0, (route, r.stderr[-3000:])
        lines = [line for line in r.stderr.splitlines() if line.startswith("Text on device: ")]
        assert len(lines) == (route != "host"), (route, r.stderr[-2000:])
        if route == "windows":
            assert int(lines[0].split()[3]) > 3
        files[route] = {f[len(route):]: (tmp_path / f).read_bytes() for f in sorted(os.listdir(tmp_path)) if f.startswith(route + ".")}
    assert len(files["host"]) >= 3 and any(k.endswith(".cz") for k in files["host"])
    assert files["device"] == files["host"] and files["windows"] == files["host"]
