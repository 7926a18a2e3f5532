"""GPU: the contig stage of bin/debruijn_contig on the MI355X against what the real reference program wrote
(tests/golden/contig_cases), and capi.ContigBuilder on hand-built tables against the restatement's serial read-out.  The steps that
load the library run in child processes under a time limit of their own (tests/contig_gpu_steps.py)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
from test_contig_cpu import BIN, CASES, SUFFIXES, golden_cases, in_order, load_case, stage_lines  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "contig_gpu_steps.py")
REF_CONSUMER = os.path.join(ROOT, "oracle", "_ref", "ref_consumer")


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def run_cli(exe, tmp_path, name, env_extra, prefix="out"):
    """-> the files the program wrote, its stderr without `Run time:` lines, the case"""
    c = load_case(name)
    (tmp_path / "reads.fa").write_bytes(c["reads"])
    lib = tmp_path / "reads.lib"
    lib.write_text(str(tmp_path / "reads.fa") + "\n")
    r = subprocess.run([exe] + c["args"] + ["-t", "1", "-o", str(tmp_path / prefix), str(lib)], capture_output=True, env=dict(os.environ, **env_extra),
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {s: open(str(tmp_path / prefix) + ".contig." + s, "rb").read() for s in SUFFIXES if os.path.exists(str(tmp_path / prefix) + ".contig." + s)}
    return got, "\n".join(ln for ln in r.stderr.decode("latin-1").split("\n") if "Run time:" not in ln), c


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_cases())
def test_cli_matches_the_reference(tmp_path, name):
    """fails on a build without the contig stage: no *.contig.seq.fa is written"""
    got, err, c = run_cli(os.path.join(BIN, "debruijn_contig"), tmp_path, name, {"DBGK_LAYOUT": "ref"})
    assert sorted(got) == sorted(c["files"])
    for s in got:
        assert got[s] == c["files"][s], (name, s)
    assert in_order(stage_lines(c["stderr"]), err + "\n") is None


@pytest.mark.gpu
def test_builder_equals_the_serial_read_out_on_hand_built_tables():
    res = run_step("tables", 300)
    print(res)
    assert all(v["host_contigs"] == 0 for name, v in res.items() if name != "palindrome")
    assert "every_flip" in res and "no_flip" in res and res["palindrome"]["contigs"] > 0
    assert res["chain_4097"]["rounds"] == 13 and res["chain_1"]["rounds"] == 1


@pytest.mark.gpu
def test_order_dependent_chains_go_to_the_host_walker():
    res = run_step("handoff", 300)
    print(res)
    assert sorted(res) == ["cycle", "key0", "non_mutual", "self_loop"] and all(v["host_contigs"] > 0 for v in res.values())


@pytest.mark.gpu
def test_hand_off_is_zero_where_the_reference_meets_no_such_structure():
    res = run_step("goldens", 300)
    print(res)
    assert len(res) == 10
    for name, v in res.items():
        if name[0] not in "gh":
            assert v["host_contigs"] == 0 and v["kernel_contigs"] == v["contigs"] > 0, (name, v)
    assert res["g_circle"]["host_contigs"] == 1


@pytest.mark.gpu
def test_default_layout_equals_the_restatement_on_the_dumped_table(tmp_path):
    img = tmp_path / "table.img"
    got, err, c = run_cli(os.path.join(BIN, "debruijn_contig"), tmp_path, "d_bubbles", {"DBGK_DUMP_TABLE": str(img), "DBGK_LAYOUT": ""})
    t = R.Table.from_image(img.read_bytes(), c["k"])
    files, lines, _ = R.run_stage(t, R.Options.from_args(c["args"]))
    assert sorted(got) == sorted(files)
    for s in files:
        assert got[s] == files[s], s
    assert in_order([ln for ln in lines.split("\n") if ln.strip()], err + "\n") is None


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_CONSUMER), reason="oracle/_ref/ref_consumer is not built (no reference sources)")
def test_live_reference_consumer_writes_the_same_files(tmp_path):
    """a genome of 5 kb with a repeat, 20x, made here: both programs at the reference's layout"""
    import random
    rng = random.Random(5)
    g = "".join(rng.choices("ACGT", k=4800))
    genome = g[:1500] + g[200:400] + g[1500:]
    comp = str.maketrans("ACGT", "TGCA")
    reads = []
    for i in range(len(genome) * 20 // 100):
        p = min(max(rng.randrange(-50, len(genome) - 50), 0), len(genome) - 100)
        r = genome[p:p + 100]
        reads.append(">r%d\n%s\n" % (i, r if rng.random() < 0.5 else r.translate(comp)[::-1]))
    (tmp_path / "reads.fa").write_text("".join(reads))
    (tmp_path / "reads.lib").write_text(str(tmp_path / "reads.fa") + "\n")
    out = {}
    for name, exe in (("ours", os.path.join(BIN, "debruijn_contig")), ("theirs", REF_CONSUMER)):
        r = subprocess.run([exe, "-k", "31", "-r", "150", "-f", "2", "-t", "1", "-i", "0.00005", "-M", "100", "-o", str(tmp_path / name),
                            str(tmp_path / "reads.lib")], capture_output=True, env=dict(os.environ, DBGK_LAYOUT="ref"), timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out[name] = {s: open(str(tmp_path / name) + ".contig." + s, "rb").read() for s in SUFFIXES}
    assert out["ours"] == out["theirs"]
    assert out["ours"]["seq.fa"].count(b">") >= 2 and b"branch" in out["ours"]["seq.fa"]
