"""GPU: the alignments of the bubble arms.  capi.ContigBuilder.align over tests/golden/align_cases/pairs.npz against what the
reference's global_aligning() returned, byte for byte (tests/align_gpu_steps.py, child processes under their own time limits), and the
contig stage of bin/debruijn_contig with its alignments computed on the GPU against what the real reference program wrote: the three
cases of tests/golden/align_cases, d_bubbles and the six ordering cases of tests/golden/simplify_cases -- as the product runs it, on
128-bit keys, in batches of one pair, with nothing submitted, and with every result made stale."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_contig_cpu import BIN, SUFFIXES, in_order, stage_lines  # noqa: E402
import contig_restatement as R  # noqa: E402
from test_align_cpu import CASE_FILES, check_stated_conditions, restated  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "align_gpu_steps.py")
ALIGN_LINE = re.compile(r"Contig stage aligned arms \(bubbles\): candidates (\d+) submitted (\d+) too long (\d+) used (\d+) aligned on the host (\d+) "
                        r"device ms (\S+) bytes copied back (\d+)\n")
# variant -> (test hooks, how the restatement is asked)
VARIANTS = {"product": ("", {}), "wide": ("contig_wide=1", {}), "batch1": ("align_batch=1", {}), "host": ("align_host=1", {"host": True}),
            "stale": ("align_stale=1", {"stale": True})}


def run_step(name, mode, timeout=120):
    r = subprocess.run([sys.executable, STEPS, name, mode], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def run_cli(tmp_path, name, hooks, timings=True):
    """-> the files the program wrote, its stderr without `Run time:` lines, the case"""
    c = R.load_case(CASE_FILES[name])
    (tmp_path / "reads.fa").write_bytes(c["reads"])
    lib = tmp_path / "reads.lib"
    lib.write_text(str(tmp_path / "reads.fa") + "\n")
    env = dict(os.environ, DBGK_LAYOUT="ref")
    if timings:
        env["DBGK_TIMINGS"] = "1"
    if hooks:
        env["DBGK_TEST_HOOKS"] = hooks
    r = subprocess.run([os.path.join(BIN, "debruijn_contig")] + c["args"] + ["-t", "1", "-o", str(tmp_path / "out"), str(lib)], capture_output=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {s: open(str(tmp_path / "out") + ".contig." + s, "rb").read() for s in SUFFIXES if os.path.exists(str(tmp_path / "out") + ".contig." + s)}
    return got, "\n".join(ln for ln in r.stderr.decode("latin-1").split("\n") if "Run time:" not in ln), c


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bare", "table", "wide"])
def test_align_equals_global_aligning_byte_for_byte(mode):
    """fails on a build without the alignment calls: ContigBuilder has no align().  Rows (lengths, score, aligned length, diffs,
    status) and both aligned strings of every pair, in one batch and in batches of 3; pairs over the bound come back TOO_LONG with
    zeros"""
    res = run_step("pairs", mode)
    print(res)
    assert res["pairs"] >= 200 and res["batches"] == 1 and res["batches_of_3"] == res["launches_for_3"] >= 70 and res["cells"] > 0


@pytest.mark.gpu
def test_argument_errors_come_before_device_work():
    assert run_step("arguments", "bare")["argument_checks"] == 9


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(CASE_FILES))
def test_stage_with_device_alignments_writes_the_reference_files(tmp_path, name, variant):
    """the eight files and the stage's stderr lines, byte for byte, in every mode; the new line's five counts are the restated rule's
    (the line itself is missing on a build without the feature); the stated conditions on them hold"""
    hooks, mode = VARIANTS[variant]
    got, err, c = run_cli(tmp_path, name, hooks)
    assert sorted(got) == sorted(c["files"])
    for s in got:
        assert got[s] == c["files"][s], (name, variant, s)
    assert in_order(stage_lines(c["stderr"]), err + "\n") is None
    lines = ALIGN_LINE.findall(err + "\n")
    assert len(lines) == 1, err[-2000:]
    counts = dict(zip(("candidates", "submitted", "too_long", "used", "host"), (int(v) for v in lines[0][:5])))
    print(name, variant, counts, lines[0][5:])
    want = restated(name, **mode)[0]["aligned"]
    assert counts == want, (name, variant, counts, want)
    if variant in ("product", "wide", "batch1"):
        check_stated_conditions(name, counts)
        assert (int(lines[0][6]) > 0) == (counts["submitted"] > 0)
    else:
        assert counts["used"] == 0 and counts["host"] == restated(name)[0]["aligned"]["used"] + restated(name)[0]["aligned"]["host"]
    if variant == "host":
        assert counts["submitted"] == 0 and int(lines[0][6]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a_indel_lengths", "c_indel_after_bubble"])
def test_stage_is_silent_about_alignments_where_the_parent_was(tmp_path, name):
    """without DBGK_TIMINGS there is no new line; with simplify_host=1 there are no traces, nothing is submitted and no line is
    printed either: the program behaves as it did before"""
    for hooks, timings in (("", False), ("simplify_host=1", True)):
        got, err, c = run_cli(tmp_path, name, hooks, timings)
        for s in got:
            assert got[s] == c["files"][s], (name, hooks, s)
        assert in_order(stage_lines(c["stderr"]), err + "\n") is None
        assert "aligned arms" not in err
