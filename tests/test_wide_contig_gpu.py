"""GPU: the contig stage on 128-bit keys (debruijn_contig -k 33..63, capi.ContigBuilder(wide=True)).  PARITY UNPINNED above k = 32: the
reference stops at k = 31.  What anchors the stage: run at k <= 31 on the reference's tables with a high word of 0 (test hook
contig_wide) it must write the reference's files byte for byte (tests/golden/contig_cases); above k = 32 it is compared with the
restatement given the 128-bit hash rule (tests/wide_contig_restatement.py).  The steps that load the library run in child processes
under a time limit of their own (tests/wide_contig_gpu_steps.py)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
import wide_contig_restatement as W  # noqa: E402
from test_contig_cpu import BIN, SUFFIXES, golden_cases, in_order, stage_lines  # noqa: E402
from test_contig_gpu import run_cli  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "wide_contig_gpu_steps.py")
WIDE_LINE = "Contig stage on 128-bit k-mers (32-byte nodes; parity unpinned above k = 32)"


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_cases())
def test_anchor_wide_stage_writes_the_reference_files_at_k_up_to_31(tmp_path, name):
    """the wide stage on the reference's table with a high word of 0; fails on a build without it: the hook is unknown there and the
    line that says the wide stage ran is missing"""
    got, err, c = run_cli(os.path.join(BIN, "debruijn_contig"), tmp_path, name, {"DBGK_LAYOUT": "ref", "DBGK_TEST_HOOKS": "contig_wide=1"})
    assert WIDE_LINE + "\n" in err, "the stage on 128-bit k-mers did not run"
    assert sorted(got) == sorted(c["files"])
    for s in got:
        assert got[s] == c["files"][s], (name, s)
    assert in_order(stage_lines(c["stderr"]), err + "\n") is None


@pytest.mark.gpu
def test_wide_builder_equals_the_serial_read_out_on_chains_parity_unpinned_above_32():
    res = run_step("tables", 120)
    assert len(res) == 40 and all(v["host_contigs"] == 0 and v["kernel_contigs"] == 1 for v in res.values())
    for k in (31, 32, 33, 48, 63):
        # the jump kernels are shared with the 64-bit read-out: its figures hold
        assert res["k%d_chain_4097" % k]["rounds"] == 13 and res["k%d_chain_1" % k]["rounds"] == 1


@pytest.mark.gpu
def test_wide_builder_equals_the_serial_read_out_on_hand_built_shapes_parity_unpinned_above_32():
    res = run_step("shapes", 120)
    print(res)
    assert all(v["host_contigs"] == 0 for name, v in res.items() if name != "palindrome")
    assert all("k%d_no_flip" % k in res for k in (31, 32, 33, 48, 63)) and all("k%d_every_flip" % k in res for k in (31, 33, 63))
    assert res["palindrome"]["contigs"] > 0
    assert all(name in res for name in ("k33_many", "k63_many", "k33_wrap", "k63_wrap", "k63_repeat"))


@pytest.mark.gpu
def test_order_dependent_chains_of_63_mers_go_to_the_host_walker():
    res = run_step("handoff", 120)
    print(res)
    assert sorted(res) == ["cycle", "key0", "non_mutual", "self_loop"] and all(v["host_contigs"] > 0 for v in res.values())


@pytest.mark.gpu
def test_wide_builder_equals_the_narrow_builder_at_k_31():
    res = run_step("narrow", 120)
    assert res["k31"]["host_contigs"] > 0 and res["k31"]["kernel_contigs"] > 4


@pytest.fixture(scope="module")
def cli_reads_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_cli")
    genome, reads = W.cli_reads()
    (d / "reads.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    (d / "reads.lib").write_text(str(d / "reads.fa") + "\n")
    return d / "reads.lib"


@pytest.mark.gpu
@pytest.mark.parametrize("k", [33, 47, 63])
def test_cli_above_32_equals_the_restatement_on_the_dumped_table_parity_unpinned(tmp_path, cli_reads_file, k):
    """debruijn_contig -k 33..63 at the default layout: the table it dumps (32-byte nodes) goes through the restatement, which gives
    the expected files and stderr lines.  Fails on a build without the stage on 128-bit keys: no *.contig.seq.fa is written.  The
    input is checked on the CPU (tests/test_wide_contig_cpu.py: at least 2 tips, 2 low-coverage edges, 3 bubbles, 4 contigs with 4
    branch ends on a table laid out in Python); the program's table has other slots and so another list order, which may move a
    structure from one pass to another, so here every pass must have removed at least one and at least two contigs come out, one
    of them ending on a branch."""
    img, prefix = tmp_path / "table.img", str(tmp_path / "out")
    args = ["-k", str(k)] + W.CLI_ARGS
    r = subprocess.run([os.path.join(BIN, "debruijn_contig")] + args + ["-o", prefix, str(cli_reads_file)], capture_output=True,
                       env=dict(os.environ, DBGK_DUMP_TABLE=str(img), DBGK_LAYOUT=""), timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    err = "\n".join(ln for ln in r.stderr.decode("latin-1").split("\n") if "Run time:" not in ln)
    assert WIDE_LINE + "\n" in err
    got = {s: open(prefix + ".contig." + s, "rb").read() for s in SUFFIXES if os.path.exists(prefix + ".contig." + s)}
    t = W.WideTable.from_image(img.read_bytes(), k)
    assert any(x >> 64 for x in t.kmer)
    files, lines, _ = W.run_stage(t, R.Options.from_args(args))
    assert sorted(got) == sorted(files) == sorted(SUFFIXES)
    for s in files:
        assert got[s] == files[s], (k, s)
    assert in_order([ln for ln in lines.split("\n") if ln.strip()], err + "\n") is None
    n = W.stage_counts(lines, files)
    print(k, n)
    assert n["tip"] >= 1 and n["lowCovEdge"] >= 1 and n["bubble"] >= 1 and n["contigs"] >= 2 and n["branch_ends"] >= 1, n
    for word in ("finished !", "Assembly completely finished!"):
        assert word in err
