"""CPU: the corrector's output stage.  Its numpy restatement (tests/corr_compact_restatement.py) applied to what
tests/correct_restatement.py computes gives, for every golden the real reference wrote, exactly the sequence lines of the
.correct.fa.gz and the numbers of the .correct.stat; the argument checks of the new entry points; the binding."""
import ctypes
import gzip
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import corr_compact_restatement as CC  # noqa: E402
import correct_edge_cases as E  # noqa: E402
import correct_restatement as CR  # noqa: E402
from test_correct_cpu import GOLDEN, expected_fa, golden_cases, params_of  # noqa: E402

EDGES = os.path.join(GOLDEN, "correct_edges")
PINNED = [s.name for s in E.scenarios() if s.pinned]


def pack(seqs):
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offsets


def check_against_reference(outs, rows, fa, stat_text):
    """outs: every read after correction, untrimmed; rows: its record fields"""
    out, offsets = pack(outs)
    bases, coff, cnt = CC.compact(out, offsets, CC.records_of(rows))
    assert CC.as_lines(bases, coff) == CC.sequence_lines(fa)
    assert CC.stat_of(cnt, int(offsets[-1])) == CC.stat_numbers(stat_text)
    assert cnt["node_limit_hits"] == sum(r[5] for r in rows)
    return cnt


@pytest.mark.parametrize("d,case", golden_cases(), ids=lambda v: v if isinstance(v, str) else v["name"])
def test_compaction_of_the_restatement_gives_the_golden_sequences_and_stat(d, case):
    from oracle import oracle_py as orc
    D = os.path.join(GOLDEN, d)
    P = params_of(case)
    bits, _ = orc.kfreq_load_1bit(os.path.join(D, "table.cz"), P.k)
    T = CR.Table(bits, P.k)
    outs, rows = [], []
    for _, seq in CR.read_records(os.path.join(D, case["reads"]), case["format"]):
        read, one, multi, deleted, lt, rt, hits = CR.correct_one_read(seq, T, P)
        outs.append(read)
        rows.append((one, multi, deleted, lt, rt, hits))
    cnt = check_against_reference(outs, rows, expected_fa(d, case), open(os.path.join(D, case["name"] + ".correct.stat")).read())
    assert cnt["node_limit_hits"] == case["node_limit_hits"]


@pytest.mark.parametrize("name", PINNED)
def test_compaction_of_the_edge_scenarios_gives_the_golden_sequences_and_stat(name):
    rs = E.restated(name)
    cnt = check_against_reference([r["out"] for r in rs], [(r["one_base"], r["tree"], r["deleted"], r["lt"], r["rt"], r["hits"], r["path"]) for r in rs],
                                  gzip.open(os.path.join(EDGES, name + ".correct.fa.gz"), "rb").read(),
                                  open(os.path.join(EDGES, name + ".correct.stat")).read())
    paths = [r["path"] for r in rs]
    assert (cnt["by_classify"], cnt["by_correct"], cnt["by_overflow"]) == (paths.count(0), paths.count(1), paths.count(2))


def test_the_trim_clamp_golden_holds_the_combination_the_length_rule_clamps():
    """left_trim == L on a deleted read: the only way the kernels' records reach left_trim + right_trim >= L (a kept read has
    L - lt - rt >= r >= 0); records from elsewhere that trim more than the read holds give 0, never a wrapped length"""
    (r,), s = E.restated("trim_clamp"), E.scenario("trim_clamp")
    assert r["deleted"] == 1 and r["lt"] == len(s.reads[0]) and r["rt"] == 0
    offsets = np.array([0, 45, 90, 135], dtype=np.uint64)
    rec = CC.records_of([(0, 0, 1, 45, 0, 0), (0, 0, 0, 30, 15, 0), (0, 0, 0, 40, 40, 0)])
    assert CC.out_lengths(offsets, rec).tolist() == [0, 0, 0]
    rec = CC.records_of([(0, 0, 0, 0, 0, 0), (0, 0, 0, 30, 14, 0), (0, 0, 1, 0, 0, 0)])
    assert CC.out_lengths(offsets, rec).tolist() == [45, 1, 0]


def test_null_arguments_are_refused_before_any_device_work():
    from dbg_assembly_amd import capi
    L = capi.lib()
    info = capi.CorrCompactInfo()
    p, u = ctypes.c_void_p(), ctypes.c_uint64()
    off = (ctypes.c_uint64 * 1)(0)
    assert L.dbgk_corr_compact(None, ctypes.byref(info)) == capi.ERR_ARG
    assert L.dbgk_corr_compact_from(None, None, off, None, 0, ctypes.byref(info)) == capi.ERR_ARG
    assert L.dbgk_corr_compact_results(None, None, None) == capi.ERR_ARG
    assert L.dbgk_corr_compact_device(None, ctypes.byref(p), ctypes.byref(p), ctypes.byref(u), ctypes.byref(u)) == capi.ERR_ARG
    assert L.dbgk_corr_reads_device(None, None, off, 0, None) == capi.ERR_ARG
    assert L.dbgk_push_corrected(None, None) == capi.ERR_ARG


def test_binding_covers_the_output_stage():
    from dbg_assembly_amd import capi
    names = {s[0] for s in capi.SYMBOLS}
    for n in ("dbgk_corr_reads_device", "dbgk_corr_compact", "dbgk_corr_compact_from", "dbgk_corr_compact_results",
              "dbgk_corr_compact_device", "dbgk_push_corrected"):
        assert n in names and hasattr(capi.lib(), n)
    assert ctypes.sizeof(capi.CorrCompactInfo) == 12 * 8 + 2 * 8
    assert [f for f, _ in capi.CorrCompactInfo._fields_][:12] == list(CC.COUNTERS)
    assert CC.REC_DTYPE == capi.CORR_REC_DTYPE
    header = open(os.path.join(ROOT, "include", "dbgk.h")).read()
    assert "#define DBGK_CORR_COMPACT_TILE %d\n" % capi.CORR_COMPACT_TILE in header
    assert capi.CORR_COMPACT_TILE % 16 == 0 and capi.lib().dbgk_abi_version() == 7
    for m in ("correct_device", "compact", "compact_from", "compact_to_host", "compact_device"):
        assert callable(getattr(capi.Corrector, m))
    assert callable(capi.Graph.push_corrected)
