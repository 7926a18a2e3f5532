"""GPU: the corrector's kernels on the edge scenarios (tests/correct_edge_cases.py) -- per read the output bytes and every
field of the record, the batch counters that say which kernel finished the read, and the table counts.  The yardstick of a
pinned scenario is the text the real reference wrote (tests/golden/correct_edges) plus the restatement for the fields the file
does not show; an unpinned one (k = 1, k = 19, bytes that the reference indexes out of bounds with) has the restatement alone.
Each GPU step is a child process under a time limit of its own; the limits only end a stuck step."""
import gzip
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import correct_edge_cases as E  # noqa: E402
from test_correct_cpu import EXE  # noqa: E402
from test_correct_gpu import run_step  # noqa: E402

EDGES = os.path.join(ROOT, "tests", "golden", "correct_edges")


def expect_all(res, names):
    assert sorted(res) == sorted(names)
    for name in names:
        s = E.scenario(name)
        paths = [r["path"] for r in E.restated(name)]
        assert res[name]["reads"] == len(s.reads) and res[name]["paths"] == [paths.count(v) for v in (0, 1, 2)]


@pytest.mark.gpu
def test_edges_k13_and_below_reference_pinned_but_k1_and_odd_bytes_restatement_only():
    res = run_step("edges_small", 120)
    print(res)
    expect_all(res, [s.name for s in E.scenarios() if s.k <= 13])
    assert res["mask_words"]["extra"]                                    # the batch shapes ran
    assert res["frontier_cap_k9_M255"]["paths"] == [0, 1, 0] and res["frontier_cap_k9_M258"]["paths"] == [0, 0, 1]
    assert res["frontier_cap_k13_M255"]["paths"] == [0, 1, 0] and res["frontier_cap_k13_M258"]["paths"] == [0, 0, 1]
    assert res["lds_length"]["paths"] == [0, 4, 2]


@pytest.mark.gpu
def test_edges_one_base_chunks_k15_16_17_reference_pinned():
    res = run_step("edges_chunks", 120)
    print(res)
    expect_all(res, ["one_base_chunks_k%d" % k for k in (15, 16, 17)])


@pytest.mark.gpu
def test_edges_k19_restatement_only_parity_unpinned_and_seal_beyond_2_32():
    res = run_step("edges_k19", 300)
    print(res)
    expect_all(res, ["k19_parity_unpinned"])
    lo, hi = res["k19_parity_unpinned"]["extra"]
    assert lo < 1 << 32 <= hi


@pytest.mark.gpu
def test_cli_matches_golden_on_mask_words(tmp_path):
    import subprocess
    meta = next(c for c in json.load(open(os.path.join(EDGES, "cases.json"))) if c["name"] == "mask_words")
    reads = tmp_path / "mask_words.fa"
    reads.write_bytes(gzip.open(os.path.join(EDGES, meta["reads"]), "rb").read())
    (tmp_path / "reads.lib").write_text("\t%s \n\n" % reads)
    r = subprocess.run([EXE] + meta["args"] + [os.path.join(EDGES, meta["table"]), str(tmp_path / "reads.lib")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert gzip.open(str(reads) + ".correct.fa.gz", "rb").read() == gzip.open(os.path.join(EDGES, "mask_words.correct.fa.gz"), "rb").read()
    assert open(str(reads) + ".correct.stat").read() == open(os.path.join(EDGES, "mask_words.correct.stat")).read()
    assert r.stderr.count("node_vec_pos exceed Max_node_in_BB_tree") == meta["node_limit_hits"]
    assert "Kmer_hifreq_num   %d\n" % meta["hifreq"] in r.stderr
