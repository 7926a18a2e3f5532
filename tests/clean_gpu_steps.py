"""GPU steps of tests/test_clean_gpu.py, each run in a child process of its own under a time limit:
    python tests/clean_gpu_steps.py capi_goldens | large
Prints one JSON line of findings; exits non-zero on a mismatch."""
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_restatement as CR  # noqa: E402
from test_clean_cpu import CASES, golden_cases  # noqa: E402


def bits(x):
    return struct.pack("<d", x)


def same_blocks(got, want):
    """dbgk_lowqual_block against the restatement's tuple: error_sum as a bit pattern"""
    return bits(got[0]) == bits(want[0]) and tuple(got[1:4]) == tuple(want[1:4])


def capi_goldens():
    """every golden case through capi.Cleaner: the numbers equal the restatement's field for field, the text equals the golden; and
    a contaminant set too large for the LDS form"""
    from dbg_assembly_amd import capi
    res = {}
    with capi.Cleaner() as c:
        for case in golden_cases():
            o = CR.case_options(case)
            recs = CR.load_reads(os.path.join(CASES, case["input"]))
            want_text = CR.expected_outputs(CASES, case)
            want = CR.run_case(CASES, case)["numbers"]
            if case["program"] == "clean_adapter":
                adapters = CR.case_adapters(CASES, case)
                c.set_adapters([s for _, s in adapters], o["-s"])
                out, hits = c.trim_adapter(recs, [n for n, _ in adapters], o["-r"])
                got = [tuple(h) for h in hits.tolist()]
                for n, (g, w) in enumerate(zip(got, want)):
                    assert g == tuple(w), (case["name"], n, g, w)
                text = CR.clean_adapter(recs, adapters, o["-s"], o["-r"], got)
            else:
                out, blocks = c.trim_lowqual(recs, o["-e"], o["-q"], o["-r"])
                got = [tuple(b) for b in blocks.tolist()]
                for n, (g, w) in enumerate(zip(got, want)):
                    assert same_blocks(g, w), (case["name"], n, g, w)
                text = CR.clean_lowqual(recs, o["-e"], o["-q"], o["-r"], got)
            assert len(got) == len(want) == len(recs)
            assert "".join("%s\n%s\n+\n%s\n" % r for r in out) == want_text["out"], case["name"]
            assert text[0] == want_text["out"] and text[1] == want_text["stat"], case["name"]
            st = c.batch_stats()
            if case["program"] == "clean_adapter":
                assert st["by_lds"] + st["by_global"] == len(recs) == st["reads"], st
                assert st["hits"] == sum(1 for g in got if g[0] >= 0), st
            res[case["name"]] = {k: st[k] for k in ("reads", "by_lds", "by_global", "hits", "cells")}
        # 40 contaminants of 130 bases: 5 200 codes do not fit the LDS form, every read goes through global memory
        rng = np.random.default_rng(11)
        contam = ["".join(rng.choice(list("ACGT"), 130)) for _ in range(40)]
        reads = []
        for n in range(300):
            s = "".join(rng.choice(list("ACGT"), int(rng.integers(1, 400))))
            if n % 3 == 0:
                s += contam[int(rng.integers(40))][:int(rng.integers(5, 60))]
            reads.append(s.encode())
        c.set_adapters(contam, 10)
        got = [tuple(h) for h in c.adapter(*capi.concat_sequences(reads)).tolist()]
        st = c.batch_stats()
        assert st["by_lds"] == 0 and st["by_global"] == len(reads), st
        want = CR.align_many(reads, [(str(n), s) for n, s in enumerate(contam)], 10)
        assert got == want, [n for n in range(len(reads)) if got[n] != want[n]][:5]
        res["large_set"] = {k: st[k] for k in ("reads", "by_lds", "by_global", "hits", "cells")}
    return res


def synthetic_job(n_reads, seed=3):
    """reads of mixed lengths (a few beyond the LDS slice), about one in ten with a contaminant prefix at its tail with 5 %
    substitutions; six contaminants, both strands"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    contam = []
    for n, length in enumerate((33, 32, 8, 58, 21, 47)):
        seq = letters[rng.integers(0, 4, length)].tobytes().decode()
        if n == 3:
            seq = seq[:20] + "N" + seq[21:]
        contam.append(("c%d" % n, seq))
    adapters = []
    for name, seq in contam:
        adapters += [(name, seq), (name + " minus-strand", CR.reverse_complement(seq))]
    lengths = rng.choice([36, 76, 100, 125, 150, 151, 250, 600], n_reads, p=[.05, .1, .15, .1, .3, .1, .15, .05])
    lengths[rng.choice(n_reads, n_reads // 500, replace=False)] = rng.integers(1025, 2001, n_reads // 500)
    lengths[rng.choice(n_reads, 20, replace=False)] = [0, 1, 2, 1023, 1024] * 4
    reads = []
    for n in range(n_reads):
        s = letters[rng.integers(0, 4, int(lengths[n]))]
        if n % 10 == 0 and len(s) > 40:
            ad = np.frombuffer(adapters[int(rng.integers(len(adapters)))][1].encode(), dtype=np.uint8).copy()
            ad = ad[:int(rng.integers(6, len(ad) + 1))]
            sub = rng.random(len(ad)) < 0.05
            ad[sub] = letters[rng.integers(0, 4, int(sub.sum()))]
            s = np.concatenate([s[:len(s) - len(ad)], ad])
        if n % 97 == 0 and len(s):
            s = s.copy()
            s[rng.integers(0, len(s), 3)] = ord("N")
        if n % 211 == 0:
            s = np.frombuffer(s.tobytes().lower(), dtype=np.uint8)
        reads.append(s.tobytes())
    return reads, adapters


def large():
    """120 000 reads: every read against the restatement, and the same job in batches of 1 000, of 64 K and in one go"""
    from dbg_assembly_amd import capi
    n_reads, cutoff = 120000, 10
    reads, adapters = synthetic_job(n_reads)
    bases, offsets = capi.concat_sequences(reads)
    rng = np.random.default_rng(9)
    quals = (33 + rng.choice([40, 40, 40, 41, 37, 30, 20, 12, 2], bases.size, p=[.3, .2, .1, .1, .1, .08, .06, .04, .02])).astype(np.uint8)
    res = {"reads": n_reads}
    with capi.Cleaner() as c:
        c.set_adapters([s for _, s in adapters], cutoff)
        whole = c.adapter(bases, offsets)
        st = c.batch_stats()
        assert st["by_lds"] > 0 and st["by_global"] > 0 and st["by_lds"] + st["by_global"] == n_reads, st
        res.update(by_lds=st["by_lds"], by_global=st["by_global"], hits=st["hits"], ms_lds=st["ms_lds"], ms_global=st["ms_global"])
        whole_q = c.lowqual(bases, quals, offsets, 0.001, 33)
        res["ms_lowqual"] = c.batch_stats()["ms_lowqual"]
        for step in (1000, 65536):
            parts, parts_q = [], []
            for a in range(0, n_reads, step):
                o = offsets[a:min(n_reads, a + step) + 1]
                lo, hi = int(o[0]), int(o[-1])
                parts.append(c.adapter(bases[lo:hi], o - o[0]))
                parts_q.append(c.lowqual(bases[lo:hi], quals[lo:hi], o - o[0], 0.001, 33))
            assert np.array_equal(np.concatenate(parts), whole), "hits depend on the batch size (%d)" % step
            assert np.concatenate(parts_q).tobytes() == whole_q.tobytes(), "blocks depend on the batch size (%d)" % step
    want = CR.align_many(reads, adapters, cutoff)
    got = [tuple(h) for h in whole.tolist()]
    bad = [n for n in range(n_reads) if got[n] != want[n]]
    assert not bad, (len(bad), bad[:5], [(got[n], want[n]) for n in bad[:3]])
    table = CR.error_table(33)
    qs = quals.tobytes().decode("latin-1")
    got_q = whole_q.tolist()
    bad = []
    for n in range(n_reads):
        lo, hi = int(offsets[n]), int(offsets[n + 1])
        w = CR.lowqual_block(reads[n].decode("latin-1"), qs[lo:hi], 0.001, 33, table)
        if not same_blocks(got_q[n], w):
            bad.append((n, got_q[n], w))
    assert not bad, (len(bad), bad[:3])
    res["trimmed"] = int(whole_q["trimmed"].sum())
    return res


if __name__ == "__main__":
    print(json.dumps({"capi_goldens": capi_goldens, "large": large}[sys.argv[1]]()))
