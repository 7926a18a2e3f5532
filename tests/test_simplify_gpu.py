"""GPU: the traced simplification paths.  capi.ContigBuilder.trace / trace_branches / update on hand-built tables against the
restatement's get_linear_path, every field (tests/simplify_gpu_steps.py, child processes under their own time limits), and the contig
stage of bin/debruijn_contig with its paths traced on the GPU against what the real reference program wrote
(tests/golden/contig_cases, and the six ordering cases of tests/golden/simplify_cases): as the product runs it, on 128-bit keys, in batches of 3 requests and with every path walked on the host."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_contig_cpu import BIN, golden_cases, in_order, stage_lines  # noqa: E402
from test_contig_cpu import SUFFIXES  # noqa: E402
import contig_restatement as R  # noqa: E402
import simplify_restatement as S  # noqa: E402

NEW_CASES = os.path.join(ROOT, "tests", "golden", "simplify_cases")
# name -> file: the ten cases of the contig stage and the six in which a removal reaches into a later walk of its pass
CASE_FILES = {n: os.path.join(ROOT, "tests", "golden", "contig_cases", n + ".npz") for n in golden_cases()}
CASE_FILES.update({f[:-4]: os.path.join(NEW_CASES, f) for f in os.listdir(NEW_CASES) if f.endswith(".npz")})
PASSES = {"tips": "-T", "low edges": "-W", "bubbles": "-B"}
_expected = {}


def run_cli(exe, tmp_path, name, env_extra):
    """-> the files the program wrote, its stderr without `Run time:` lines, the case"""
    c = R.load_case(CASE_FILES[name])
    (tmp_path / "reads.fa").write_bytes(c["reads"])
    lib = tmp_path / "reads.lib"
    lib.write_text(str(tmp_path / "reads.fa") + "\n")
    r = subprocess.run([exe] + c["args"] + ["-t", "1", "-o", str(tmp_path / "out"), str(lib)], capture_output=True, env=dict(os.environ, **env_extra),
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {s: open(str(tmp_path / "out") + ".contig." + s, "rb").read() for s in SUFFIXES if os.path.exists(str(tmp_path / "out") + ".contig." + s)}
    return got, "\n".join(ln for ln in r.stderr.decode("latin-1").split("\n") if "Run time:" not in ln), c


def expected_counts(name, c):
    """{pass: (requests, traces used, fell back)} as the three-condition rule gives them in Python; computed once per case"""
    if name not in _expected:
        _expected[name] = S.run_passes(R.Table.from_case(c), R.Options.from_args(c["args"]))[1]
    return _expected[name]


STEPS = os.path.join(ROOT, "tests", "simplify_gpu_steps.py")
PASS_LINE = re.compile(r"Contig stage traced paths \((tips|low edges|bubbles)\): requests (\d+) traces used (\d+) fell back to the host walk (\d+) "
                       r"device ms (\S+) bytes copied back (\d+)")


def run_step(name, mode, timeout=120):
    r = subprocess.run([sys.executable, STEPS, name, mode], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def check_trace_cases(res, ks):
    print(res)
    for k in ks:
        c = res["k%d_chain10" % k]
        # walks that stop on a linear node at the cutoff; between two dead ends no walk from a linear node runs off the chain (the
        # dead ends themselves, walked outwards, and the key-0 slot do: the start node is walked whatever it is)
        assert c["cut"] > 0 and c["absent"] > 0 and c["absent_from_linear"] == 0
        assert res["k%d_absent" % k]["absent"] > 0 and res["k%d_fork" % k]["branch"] > 0
        assert res["k%d_cycle" % k]["repeats"] > 0 and res["k%d_cycle" % k]["max_len"] == 100
        assert res["k%d_poly_a" % k]["repeats"] > 0 and res["k%d_key0" % k]["requests"] > 0
        assert ("k%d_every_flip" % k in res) == (k % 2 == 1) and ("k%d_palindrome" % k in res) == (k % 2 == 0)
        assert "k%d_no_flip" % k in res and "k%d_wrap" % k in res


def check_branch_cases(res, ks):
    print(res)
    for k in ks:
        v = res["k%d_forks" % k]
        assert all(v[f] > 0 for f in ("edges_2", "edges_3", "edges_4", "both_sides", "below", "absent", "not_linear", "flipped", "kept")), (k, v)


@pytest.mark.gpu
def test_trace_equals_get_linear_path_in_every_field():
    """fails on a build without the SIMPLIFY calls: ContigBuilder has no trace()"""
    check_trace_cases(run_step("trace", "narrow"), (21, 20, 31))


@pytest.mark.gpu
def test_wide_trace_equals_the_narrow_one_at_k_up_to_31():
    check_trace_cases(run_step("trace", "wide31"), (21, 20, 31))


@pytest.mark.gpu
def test_wide_trace_equals_the_restatement_at_k_33_47_63_parity_unpinned():
    check_trace_cases(run_step("trace", "above32"), (33, 47, 63))


@pytest.mark.gpu
def test_branch_expansion_equals_the_restatement_row_by_row():
    check_branch_cases(run_step("branches", "narrow"), (21, 20, 31))


@pytest.mark.gpu
def test_wide_branch_expansion_equals_the_narrow_one_at_k_up_to_31():
    check_branch_cases(run_step("branches", "wide31"), (21, 20, 31))


@pytest.mark.gpu
def test_wide_branch_expansion_at_k_33_47_63_parity_unpinned():
    check_branch_cases(run_step("branches", "above32"), (33, 47, 63))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["narrow", "wide31", "above32_parity_unpinned"])
def test_update_carries_host_changes_to_the_device_copy(mode):
    res = run_step("update", mode.split("_")[0])
    print(res)
    assert len(res) == 3 and all(v["differ"] > 4 for v in res.values())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["narrow", "wide31", "above32_parity_unpinned"])
def test_request_counts_batches_and_argument_checks(mode):
    res = run_step("counts", mode.split("_")[0])
    print(res)
    assert res["n0"] == 0 and res["n1"] == res["n257"] == 1 and res["batched"] == 5 and res["batched_branches"] == 2 and res["argument_checks"] == 9


VARIANTS = {"product": "", "wide": "contig_wide=1", "batch3": "simplify_batch=3", "wide_batch3": "contig_wide=1,simplify_batch=3", "host": "simplify_host=1"}


ORDERING_PASS = {"a": "tips", "b": "tips", "c": "tips", "d": "low edges", "e": "bubbles", "f": "tips"}   # simplify_cases, by first letter


def pass_lines(err):
    return {m.group(1): dict(requests=int(m.group(2)), used=int(m.group(3)), fell_back=int(m.group(4)), bytes=int(m.group(6))) for m in PASS_LINE.finditer(err)}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(CASE_FILES))
def test_stage_with_traced_paths_writes_the_reference_files(tmp_path, name, variant):
    """the eight files and the stage's stderr lines, byte for byte; with simplify_host=1 no path is traced and the same comes out.  The
    per-pass counts are the restated rule's in every traced variant: neither the key width nor the batch size changes them"""
    env = {"DBGK_LAYOUT": "ref", "DBGK_TIMINGS": "1"}
    if VARIANTS[variant]:
        env["DBGK_TEST_HOOKS"] = VARIANTS[variant]
    got, err, c = run_cli(os.path.join(BIN, "debruijn_contig"), tmp_path, name, env)
    assert sorted(got) == sorted(c["files"])
    for s in got:
        assert got[s] == c["files"][s], (name, variant, s)
    assert in_order(stage_lines(c["stderr"]), err + "\n") is None
    lines = pass_lines(err)
    print(name, variant, lines)
    o = dict(zip(c["args"][::2], c["args"][1::2]))
    enabled = [p for p, opt in PASSES.items() if o.get(opt, "1") != "0"]
    if variant == "host":
        assert lines == {} and "Contig stage traced paths" not in err
    else:
        assert sorted(lines) == sorted(enabled)
        assert {p: (v["requests"], v["used"], v["fell_back"]) for p, v in lines.items()} == expected_counts(name, c)


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", [("b_tips", "tips"), ("c_lowedge", "low edges"), ("d_bubbles", "bubbles")])
def test_stage_uses_traces(tmp_path, name, which):
    """fails on a build without tracing: there is no such line"""
    got, err, c = run_cli(os.path.join(BIN, "debruijn_contig"), tmp_path, name, {"DBGK_LAYOUT": "ref", "DBGK_TIMINGS": "1"})
    lines = pass_lines(err)
    print(lines)
    assert which in lines and lines[which]["used"] > 0 and lines[which]["bytes"] > 0
    assert c["shows"][{"tips": "tips", "low edges": "lowedges", "bubbles": "bubbles_snp"}[which]] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASE_FILES))
def test_stage_counts_equal_the_restated_rule(tmp_path, name):
    """requests, traces used and walks that fell back to the host, per pass, as the three-condition rule gives them in Python; in each
    of the six ordering cases some walk falls back, and the pass with the ordering is the one that says so"""
    got, err, c = run_cli(os.path.join(BIN, "debruijn_contig"), tmp_path, name, {"DBGK_LAYOUT": "ref", "DBGK_TIMINGS": "1"})
    counts = expected_counts(name, c)
    lines = pass_lines(err)
    print(name, lines)
    assert {p: (v["requests"], v["used"], v["fell_back"]) for p, v in lines.items()} == counts
    if name == "e_no_passes":
        assert counts == {} and lines == {}
    if CASE_FILES[name].startswith(NEW_CASES):
        assert sum(v["fell_back"] for v in lines.values()) > 0
        assert lines[ORDERING_PASS[name[0]]]["fell_back"] > 0 and lines[ORDERING_PASS[name[0]]]["used"] > 0
