"""GPU: the contig stage's first pass for k = 33..63 on the device, handed over with the table (k_wide_kmer_links,
dbgk_wide_export_host_table_links, the communicator's form, debruijn_contig -k 33..63).  PARITY UNPINNED above k = 32: everything is
compared with contig_restatement.first_pass applied to the very table that came back; `anchor` ties the pass to the 64-bit one, whose
stage output the real reference pins.  The steps that load the library run in child processes under a time limit of their own
(tests/wide_links_gpu_steps.py); the inputs are checked without a GPU in tests/test_wide_links_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
import wide_contig_restatement as W  # noqa: E402
import wide_links_gpu_steps as S  # noqa: E402

STEPS = os.path.join(ROOT, "tests", "wide_links_gpu_steps.py")
CLI = os.path.join(ROOT, "dbg_assembly_amd", "bin", "debruijn_contig")
GPU_LINE = "First pass of the contig stage done on the GPU"
NODE32 = np.dtype([("hi", "<u8"), ("lo", "<u8"), ("l", "<u4"), ("r", "<u4"), ("reserved", "<u8")])


def run_step(name, timeout):
    r = subprocess.run([sys.executable, STEPS, name], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_every_boundary_of_the_kernel_equals_the_restatement_parity_unpinned():
    """k 33 / 48 / 63 x cutoff 0 / 2 / 5 x tables of 251, 4099 and 12301 slots; capacities exact, one short, and counts only.  Fails on a
    build without the feature: the call does not exist"""
    res = run_step("shapes", 120)
    print(res)
    assert len(res) == 27
    assert all(v[0] > 0 for name, v in res.items())                                    # tips everywhere
    assert all(v[1] > 0 for name, v in res.items() if not name.endswith("cutoff 5"))   # branches where the coverage passes the cutoff
    assert all(v[2] > 1 for name, v in res.items() if name.endswith("cutoff 5"))       # deleted nodes


@pytest.mark.gpu
def test_nodes_placed_on_the_host_take_their_places_in_records_flags_lists_and_counts():
    res = run_step("placed", 120)
    print(res)
    assert len(res) == 9 and all(v[2] == 4 for v in res.values())   # three side-table nodes and the key-0 node


@pytest.mark.gpu
def test_anchor_at_k_31_the_wide_pass_equals_the_narrow_one_by_kmer():
    res = run_step("anchor", 120)
    assert sorted(res) == ["b_tips", "d_bubbles"]


# ---- debruijn_contig -k 33..63 ---------------------------------------------------------------------------------------------------
def cli_args(k, cutoff, table="0.00003"):
    args = ["-k", str(k)] + list(W.CLI_ARGS)
    args[args.index("-D") + 1] = str(cutoff)
    args[args.index("-i") + 1] = table
    return args


def run_cli(tmp_path, k, cutoff, name, env_extra, table="0.00003"):
    """-> stderr, the files <prefix>.contig.*, the path of the table image, the links dump (None when none was written)"""
    d = tmp_path / name
    d.mkdir()
    (d / "reads.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(S.placed_reads(k))))
    (d / "reads.lib").write_text(str(d / "reads.fa") + "\n")
    img, lk, prefix = d / "table.img", d / "links.txt", str(d / "out")
    env = dict(os.environ, DBGK_DUMP_TABLE=str(img), DBGK_DUMP_LINKS=str(lk), DBGK_LAYOUT="")
    env.pop("DBGK_LINKS", None)
    env.update(env_extra)
    r = subprocess.run([CLI] + cli_args(k, cutoff, table) + ["-o", prefix, str(d / "reads.lib")], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    files = {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f.startswith("out.contig.")}
    return r.stderr.decode("latin-1"), files, img, (lk.read_text() if lk.exists() else None)


def links_text(img, k, cutoff):
    """the links dump that first_pass gives for a dumped table image, in the form the program writes it.  Only occupied slots matter to
    first_pass, and it takes them in slot order, so it runs on a table that holds the occupied slots alone, in that order, and its
    list entries are mapped back to slot numbers: the same function on the same nodes, without a Python list per empty slot (the
    sharded run's table has 67 million of them)"""
    raw = np.memmap(str(img), dtype=np.uint8, mode="r")
    size = int(raw[:8].view("<u8")[0])
    nodes = raw[16:16 + 32 * size].view(NODE32)
    occ = np.flatnonzero(np.unpackbits(np.asarray(raw[16 + 32 * size:16 + 32 * size + size // 8 + 1]))[:size])
    t = W.WideTable(len(occ), k)
    for j, i in enumerate(occ):
        n = nodes[int(i)]
        t.kmer[j], t.l_link[j], t.r_link[j], t.filled[j] = (int(n["hi"]) << 64) | int(n["lo"]), int(n["l"]), int(n["r"]), True
    tips, branches, _, _ = R.first_pass(t, R.Options(D=cutoff))
    rec = [t.l_num[j] | t.l_base[j] << 2 | t.r_num[j] << 4 | t.r_base[j] << 6 | (0x100 if t.linear[j] else 0) for j in range(len(occ))]
    lines = ["#size %d tips %d branches %d" % (size, len(tips), len(branches))]
    lines += ["K\t%d\t%04x\t%d" % (occ[j], rec[j], t.deleted[j]) for j in range(len(occ))]
    lines += ["T\t%d" % occ[j] for j in tips] + ["B\t%d" % occ[j] for j in branches]
    zero_low = {int(occ[j]) for j in range(len(occ)) if t.kmer[j] & W.M64 == 0}
    return "\n".join(lines) + "\n", zero_low, [int(occ[j]) for j in tips], [int(occ[j]) for j in branches]


def check_dump(err, img, dump, k, cutoff):
    assert GPU_LINE in err, "the first pass did not run on the GPU"
    want, zero_low, tips, branches = links_text(img, k, cutoff)
    assert dump == want
    assert GPU_LINE + ": %d tip nodes, %d branching nodes\n" % (len(tips), len(branches)) in err
    assert len(zero_low) == 4 and zero_low & set(tips) and zero_low & set(branches)   # placed nodes in both lists
    return tips, branches


@pytest.mark.gpu
@pytest.mark.parametrize("k,cutoff", [(33, 1), (33, 2), (63, 1), (63, 2)])
def test_cli_hands_the_first_pass_over_with_the_table_parity_unpinned(tmp_path, k, cutoff):
    """fails on a build without the feature: stderr lacks the line and no links dump is written for -k above 32"""
    err, files, img, dump = run_cli(tmp_path, k, cutoff, "run", {})
    tips, branches = check_dump(err, img, dump, k, cutoff)
    assert len({i // S.BLOCK_SLOTS for i in tips}) > 1 and len({i // S.BLOCK_SLOTS for i in branches}) > 1
    assert len(files) == 8 and "Assembly completely finished!" in err


@pytest.mark.gpu
def test_cli_three_shards_of_one_table_the_communicators_form(tmp_path):
    """dbgk_comm_wide_export_host_table_links: the pass per shard on its slot range of a table of 67 million slots, started like
    test_gpu_cli.py starts its three shards"""
    err, files, img, dump = run_cli(tmp_path, 47, 2, "shards", {"DBGK_GPU_LIST": "0,0,0", "DBGK_BATCH_BYTES": "20000"}, table="0.0672")
    assert "over 3 GPU shards" in err
    check_dump(err, img, dump, 47, 2)
    assert len(files) == 8


@pytest.mark.gpu
def test_cli_host_pass_and_device_pass_are_interchangeable(tmp_path):
    """DBGK_LINKS=0 keeps the pass on the host: no line, no dump, and the eight files byte for byte those of the default run"""
    err, files, _, dump = run_cli(tmp_path, 63, 2, "device", {})
    assert GPU_LINE in err and dump is not None
    err0, files0, _, dump0 = run_cli(tmp_path, 63, 2, "host", {"DBGK_LINKS": "0"})
    assert GPU_LINE not in err0 and dump0 is None
    assert len(files) == 8 and sorted(files0) == sorted(files)
    for name in files:
        assert files0[name] == files[name], name
