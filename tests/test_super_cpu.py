"""CPU: link_supertig -- the command line, the argument checks of the C ABI, the binding, and the Python restatement of the program
against every golden the real reference wrote (tests/golden/super_cases)."""
import ctypes
import gzip
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fill_restatement as FR  # noqa: E402
import link_restatement as LR  # noqa: E402
import super_restatement as SR  # noqa: E402

BIN = os.path.join(ROOT, "dbg_assembly_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLDEN, "super_cases")
PROG = os.path.join(BIN, "link_supertig")


def golden_cases():
    return SR.golden_cases(CASES)


def test_cli_prints_the_reference_usage_on_stderr():
    want = open(os.path.join(GOLDEN, "super_usage.txt"), "rb").read()
    assert want.decode() == SR.usage_text()
    for args in ([], ["-h"], ["only_one_argument"]):
        r = subprocess.run([PROG] + args, capture_output=True, timeout=60)
        assert r.returncode == 0 and r.stderr == want and r.stdout == b"", args
    # (the usage shows the value -n was given so far, as the reference's does)
    r = subprocess.run([PROG, "-n", "5", "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stderr == want.replace(b"default=3", b"default=5")
    r = subprocess.run([PROG, "-x"], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stderr.endswith(want)


def test_super_entry_points_validate_before_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p()
    zero = (ctypes.c_int32 * 3)(0, 0, 0)
    good = capi.SuperParams(3, zero)
    assert L.dbgk_super_create(ctypes.byref(capi.SuperParams(-1, zero)), 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_super_create(ctypes.byref(capi.SuperParams(3, (ctypes.c_int32 * 3)(0, 1, 0))), 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_super_create(None, 0, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_super_create(ctypes.byref(good), -1, ctypes.byref(h)) == capi.ERR_ARG
    assert L.dbgk_super_create(ctypes.byref(good), 0, None) == capi.ERR_ARG
    n = ctypes.c_uint64()
    buf = (ctypes.c_uint64 * 16)()
    assert L.dbgk_super_destroy(None) == capi.ERR_ARG
    assert L.dbgk_super_set_contigs(None, buf, 1) == capi.ERR_ARG
    assert L.dbgk_super_set_reads(None, buf, buf, 1) == capi.ERR_ARG
    assert L.dbgk_super_add_records(None, buf, 1) == capi.ERR_ARG
    assert L.dbgk_super_add_hits(None, buf, 1, 0) == capi.ERR_ARG
    assert L.dbgk_super_build(None) == capi.ERR_ARG
    assert L.dbgk_super_export(None, None, None, 0, ctypes.byref(n), None) == capi.ERR_ARG
    assert L.dbgk_super_gap_stats(None, None, 0, ctypes.byref(n)) == capi.ERR_ARG
    assert L.dbgk_super_resolve(None, None) == capi.ERR_ARG
    assert L.dbgk_super_snapshot(None, 0, None, None, None) == capi.ERR_ARG
    assert L.dbgk_super_layout(None, None, None, None, None) == capi.ERR_ARG
    assert L.dbgk_super_slices(None, None, 0, ctypes.byref(n)) == capi.ERR_ARG
    assert L.dbgk_super_slice_bytes(None, None, 0, ctypes.byref(n)) == capi.ERR_ARG
    assert L.dbgk_super_emit(None, None, buf, 0, None, 0, None, 0, ctypes.byref(n)) == capi.ERR_ARG
    assert L.dbgk_super_batch_stats(None, None) == capi.ERR_ARG


def test_binding_covers_the_super_section():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    section = ("create", "destroy", "set_contigs", "set_reads", "add_records", "add_hits", "build", "export", "gap_stats", "resolve",
               "snapshot", "layout", "slices", "slice_bytes", "emit", "batch_stats")
    for n in section:
        assert "dbgk_super_" + n in names and hasattr(capi.lib(), "dbgk_super_" + n)
    assert sorted(s for s in names if s.startswith("dbgk_super_")) == sorted("dbgk_super_" + n for n in section)
    assert capi.SUPER_GAPSTAT_DTYPE.itemsize == 32 and capi.SUPER_JUNCTION_DTYPE.itemsize == 56 and capi.SUPER_SLICE_DTYPE.itemsize == 24
    assert capi.SUPER_JUNCTION_DTYPE.fields["first_slice"][1] == 40 and capi.SUPER_SLICE_DTYPE.fields["reversed"][1] == 20
    assert ctypes.sizeof(capi.SuperParams) == 16 and ctypes.sizeof(capi.SuperSummary) == 112 and ctypes.sizeof(capi.SuperTiming) == 88
    assert capi.lib().dbgk_abi_version() == 7
    for m in ("set_contigs", "set_reads", "add_records", "add_hits", "build", "resolve", "gap_stats", "layout", "slices", "emit", "timing",
              "table", "__enter__"):
        assert hasattr(capi.SuperLinker, m), m
    assert list(inspect.signature(capi.SuperLinker.__init__).parameters) == ["self", "pair_num_cut", "device"]
    assert inspect.signature(capi.SuperLinker.__init__).parameters["pair_num_cut"].default == 3
    assert list(inspect.signature(capi.SuperLinker.add_hits).parameters) == ["self", "hits", "first_read"]


def test_no_super_linker_without_gpu(tmp_path):
    """no device: the binding raises and the program exits non-zero with a message, nothing falls back to the host"""
    from dbg_assembly_amd import capi
    if capi.lib().dbgk_device_count() > 0:
        return
    with pytest.raises(capi.DbgkError) as e:
        capi.SuperLinker()
    assert e.value.status == capi.ERR_HIP
    case = next(c for c in golden_cases() if c["name"] == "n1")
    LR.unpack_inputs(CASES, case, tmp_path / "c")
    r = subprocess.run([PROG, "-o", "x", case["contigs"], case["lib"]], cwd=tmp_path / "c", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "dbgk_super_create failed" in r.stderr


def test_cli_refuses_contig_names_the_reference_cannot_index(tmp_path):
    (tmp_path / "c.fa").write_text(">ctg_1\nACGT\n>ctg_5\nACGT\n")
    (tmp_path / "p.lib").write_text("")
    r = subprocess.run([PROG, "c.fa", "p.lib"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "its number must be 3" in r.stderr


@pytest.mark.parametrize("what", ["short", "missing"])
def test_cli_names_the_read_that_has_no_slice(tmp_path, what):
    """a spanning read that is too short for its slice, or in no reads file: exit 1 with the read and the two contigs named (the
    reference aborts out of substr).  The layout comes from the device, so without one the program stops at its first device call."""
    from dbg_assembly_amd import capi
    case = next(c for c in golden_cases() if c["name"] == "n1")
    work = tmp_path / "c"
    LR.unpack_inputs(CASES, case, work)
    f = work / "part1.map_reads.2ctg.gz.reads.fa.gz"
    lines = gzip.decompress(f.read_bytes()).decode("latin-1").split("\n")
    assert lines[0] == ">read_1"                       # the first record spans ctg_1 and ctg_3, a junction of the layout
    lines[0:2] = [">read_1", lines[1][:100]] if what == "short" else []
    f.write_bytes(gzip.compress("\n".join(lines).encode("latin-1")))
    r = subprocess.run([PROG, "-n", "1", "-o", "x", case["contigs"], case["lib"]], cwd=work, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    if capi.lib().dbgk_device_count() > 0:
        assert "read read_1 that spans ctg_1 and ctg_3" in r.stderr and "dbgk_super_resolve failed" in r.stderr
    else:
        assert "dbgk_super_create failed" in r.stderr


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_golden(case):
    want = LR.expected_outputs(CASES, case)
    got, _ = SR.run_case(CASES, case)
    assert len(want) == 8
    SR.compare_outputs(case, got, want)


def test_goldens_cover_what_they_are_meant_to():
    cases = {c["name"]: c for c in golden_cases()}
    assert {SR.case_params(c).n for c in cases.values()} == {1, 2, 3, 5} and sum(c["tie"] for c in cases.values()) == 1
    assert not any("-n" in c["args"] for c in cases.values() if SR.case_params(c).n == 3)          # the default is not spelled out
    for name, case in cases.items():
        assert all(not n.endswith((".cpp", ".h", ".py", ".pl", ".sh")) and "Makefile" not in n for n in LR.case_files(CASES, case))
        assert os.path.getsize(os.path.join(CASES, name + ".zip")) <= 200 * 1024
        assert len(LR.read_lib(LR.case_files(CASES, case)[case["lib"]].decode())) == 2              # two map files in one lib
    got, res = SR.run_case(CASES, cases["n_default"])
    text = LR.expected_outputs(CASES, cases["n_default"])
    err, pos, gap = text["stderr.txt"], text["res_n_default.supertig.pos.tab"], text["res_n_default.supertig.gap.data"]
    st, c = res["stats"], res["counters"]
    J = {(j["left"], j["right"]): j for j in res["junctions"]}
    assert min(c["FR"], c["RF"], c["FF"], c["RR"]) > 0                                              # reads on both strands
    assert any(it[0] == "ctg" and it[2] for its in res["layout"] for it in its)                     # a contig laid out reversed
    assert c["wrong"] == 1 and st[(0, 1)][:5] == (121, 119, 130, 7, 2)                              # a wrong-direction line counts ...
    assert "\t3,6,720,120" in text["res_n_default.supertig.links.all"]                              # ... in the statistics only
    assert st[(4, 5)][:5] == (-3, -4, -3, 3, 0) and J[(4, 5)]["written"] == 1                       # -11 / 3 truncates toward zero
    assert "Error may happens: mean_gap_size <= 0\n" in err and "\t1\tN\t-4\t-3\t3\t0\n" in pos
    assert all(s[0] == 500 for s in J[(4, 5)]["slices"])                                            # overlaps: slices of 500 bytes
    assert st[(2, 3)][1] == 15 and st[(2, 3)][2] == 17                                              # odd gaps
    j = J[(3, 4)]                                                                                   # clamped by the end of the read
    assert sorted(s[0] for s in j["slices"] if not s[3]) == [449, 450] and sorted(s[0] for s in j["slices"] if s[3])[:2] == [451, 550]
    assert "Altert message:  gap_id %d  600\t450\n" % j["gap_id"] in err
    _, _, _, recs, _, reads = SR.load_case(CASES, cases["n_default"])
    zero = [SR.slice_geometry(int(r["align1_end"]), int(r["align2_start"]), len(reads[int(r["read"])]))[0] == 0 for r in np.concatenate(recs)]
    assert sum(zero) >= 4                                                                           # slices with pos == 0
    odd = [s for s in J[(17, 18)]["slices"] if s[2]]                                                # reversed slices of reads with n, N, lower case
    flipped_reads = [reads[int(np.concatenate(recs)[s[1]]["read"])] for s in odd]
    assert odd and all("acgtnNRYx" in r for r in flipped_reads) and all(FR.rev_com_seq("acgtnNRYx") in s[4] for s in odd)
    assert FR.rev_com_seq("acgtnNRYx") in gap
    j = J[(1, 2)]                                                                                   # the introsort path, ties of different bytes
    assert len(j["slices"]) > 16 and len({s[4] for s in j["slices"] if s[0] == 560}) >= 8
    assert len({int(np.concatenate(recs)[s[1]]["read"]) < 16 for s in j["slices"]}) == 2             # its records lie in both map files
    assert c["interleave"] == 2 and (8, 10) not in J and (8, 9) in J and (9, 10) in J               # the interleaving pass
    assert c["repeat"] == 1 and text["res_n_default.supertig_repeat.seq.fa"].startswith(">spt_")    # a repeat contig
    assert st[(19, 20)][:5] == (3, 3, 4, 1070, 0) and "\t41,1023,3069,3" in text["res_n_default.supertig.links.all"]
    assert len(J[(19, 20)]["slices"]) == 1070
    ids = [int(l.split(" ")[0][4:]) for l in gap.split("\n") if l.startswith(">gap")]
    assert ids == list(range(1, len(ids) + 1))                                                      # gap ids in walk order
    order = [int(t.split("\t")[0]) for t in pos.split("\tgap")[1:]]
    assert order != sorted(order)                                                                   # ... not in output order
    _, tie = SR.run_case(CASES, cases["n2_tie"])
    lengths = [sum(SR.item_len(it) for it in items) for items in tie["layout"]]
    assert len(set(lengths)) < len(lengths)
    _, n5 = SR.run_case(CASES, cases["n5"])
    J5 = {(j["left"], j["right"]) for j in n5["junctions"]}
    assert (4, 5) in J and (4, 5) not in J5                                                         # three records: kept by -n 3, cut by -n 5
    assert (15, 16) in J and (15, 16) not in J5                                                     # four records likewise
    assert (14, 15) not in J and (14, 15) in {(j["left"], j["right"]) for j in SR.run_case(CASES, cases["n1"])[1]["junctions"]}


def test_restatement_pieces():
    assert SR.trunc_mean(-7, 2) == -3 and SR.trunc_mean(-11, 3) == -3 and SR.trunc_mean(7, 2) == 3
    assert [SR.median_index(n) for n in (1, 2, 3, 4, 7)] == [0, 1, 1, 2, 3]
    assert not SR.keeps(450, 600) and SR.keeps(451, 600) and SR.keeps(749, 600) and not SR.keeps(750, 600)   # strict, in double
    assert not SR.keeps(3, 4) and not SR.keeps(5, 4) and SR.keeps(4, 4) and not SR.keeps(0, 0)
    assert SR.slice_geometry(400, 501, 900) == (150, 600) and SR.slice_geometry(400, 501, 600) == (150, 450)
    assert SR.slice_geometry(250, 291, 540) == (0, 540)                        # pos == 0
    assert SR.slice_geometry(400, 397, 1000) == (148, 500)                     # an overlap: no gap, 500 bytes
    assert SR.slice_geometry(400, 501, 150) == (150, 0)                        # pos == length: an empty slice
    assert SR.slice_geometry(400, 501, 149) is None and SR.slice_geometry(200, 221, 900) is None and SR.slice_geometry(400, 501, None) is None
    recs = np.zeros(4, dtype=SR.REC_DTYPE)
    recs["contig1"], recs["contig2"] = [0, 1, 0, 1], [1, 0, 1, 0]
    recs["align1_end"], recs["align2_start"] = 10, [7, 6, 7, 8]                # gaps -4 -5 -4 -3
    m = SR.gap_stats(recs)[(0, 1)]
    assert m[:5] == (-4, -5, -3, 4, 0) and m[5].tolist() == [0, 1, 2, 3]
    recs["align2_start"] = [7, 6, 7, 7]                                        # -4 -5 -4 -4: -17 / 4 = -4, deviations 0 1 0 0
    assert SR.gap_stats(recs)[(0, 1)][:5] == (-4, -5, -4, 4, 0)
    v = [(5, "a"), (7, "b"), (5, "c"), (9, "d")]
    LR.std_sort(v, LR.by_len)
    assert [x[0] for x in v] == [9, 7, 5, 5]
