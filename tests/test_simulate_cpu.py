"""CPU: simulate_lowfreq_kmer -- the Python restatement (tests/simulate_restatement.py: reader, table on both strands,
mutation scan, printing) against every golden the real reference program wrote (tests/golden/simulate_cases), the command
line's usage text and refusals, and the argument checks of the C ABI that need no device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simulate_restatement as SIM  # noqa: E402

EXE = os.path.join(ROOT, "dbg_assembly_amd", "bin", "simulate_lowfreq_kmer")
GOLDEN = os.path.join(ROOT, "tests", "golden", "simulate_cases")
CASES = json.load(open(os.path.join(GOLDEN, "cases.json")))


def options_of(case):
    o = dict(zip(case["args"][0::2], case["args"][1::2]))
    return int(o.get("-k", 17)), int(o.get("-s", 100))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_restatement_reproduces_golden(case):
    k, skip = options_of(case)
    seqs = SIM.read_genome(os.path.join(GOLDEN, case["file"]))
    assert all(len(s) >= 2 * k - 1 for s in seqs) and all(set(s) <= set(b"ACGTNacgtn") for s in seqs)
    assert SIM.report(seqs, k, skip).encode() == open(os.path.join(GOLDEN, case["name"] + ".stdout"), "rb").read()


def test_goldens_cover_the_listed_ground():
    ks = {options_of(c)[0] for c in CASES}
    assert {1, 2, 5, 9, 13, 16} <= ks
    hists = {}
    for c in CASES:
        k, skip = options_of(c)
        seqs = SIM.read_genome(os.path.join(GOLDEN, c["file"]))
        hists[c["name"]] = SIM.mutation_scan(seqs, k, skip, SIM.lookup_in_values(SIM.table_of(seqs, k)))
    assert hists["k9_polyA"][9] == hists["k9_polyA"].sum() > 0                    # every mutated window absent
    assert hists["k5_every_kmer"][0] == hists["k5_every_kmer"].sum() > 0          # every mutated window present
    assert np.count_nonzero(hists["k9_two_letters"][1:9]) >= 4 and np.count_nonzero(hists["k5_period3"][1:5]) >= 2   # middle bins
    assert hists["k9_exactly_2k_minus_1"].sum() == 1 and hists["k9_skip_beyond_sequence"].sum() == 1
    assert hists["k9_last_site_at_the_end"].sum() == hists["k9_one_base_short"].sum() + 1 == 31


def test_site_rule():
    assert [SIM.site_count(n, 9, 7) for n in (16, 17, 23, 24, 25)] == [0, 1, 1, 2, 2]
    assert SIM.site_count(17, 9, 1) == 1 and SIM.site_count(20, 9, 1) == 4


def test_cli_prints_the_reference_usage():
    want = open(os.path.join(GOLDEN, "simulate_usage.txt"), "rb").read()
    for args in ([], ["-h"], ["-k", "5"]):   # no genome file: the usage text (the reference reads a null argument there)
        r = subprocess.run([EXE] + args, capture_output=True, timeout=60)
        if args == ["-k", "5"]:
            assert r.returncode == 0 and r.stdout == want.replace(b"default=17", b"default=5")
        else:
            assert r.returncode == 0 and r.stdout == want


@pytest.mark.parametrize("opts,word", [(["-k", "19"], "1..18"), (["-k", "0"], "1..18"), (["-s", "0"], "at least 1")])
def test_cli_refuses_what_it_does_not_hold(tmp_path, opts, word):
    r = subprocess.run([EXE] + opts + [str(tmp_path / "g.fa")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and word in r.stderr and r.stdout == ""
