"""GPU steps of tests/test_map_gpu.py, each run in a child process of its own under a time limit:
    python tests/map_gpu_steps.py capi_goldens | large
Prints one JSON line of findings; exits non-zero on a mismatch."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_restatement as MR  # noqa: E402
from test_map_cpu import CASES, golden_cases  # noqa: E402


def to_hits(arr):
    return [tuple(MR.Hit(*(int(v) for v in h)) for h in pair) for pair in arr.tolist()]


def capi_goldens():
    """every golden case through capi.Mapper: hits equal the restatement's field for field, the formatted text equals the golden"""
    from dbg_assembly_amd import capi
    res = {}
    for case in golden_cases():
        stats = {"by_lds": 0, "by_long": 0, "skipped": 0, "windows_probed": 0, "reads": 0}

        def mapper(X, reads, P, second):
            with capi.Mapper(k=P.k, s=P.s, r=P.r, identity=P.i, second_alignment=second) as m:
                m.set_contigs(X.contigs)
                got = to_hits(m.map_sequences(reads))
                st = m.batch_stats()
            for key in stats:
                stats[key] += st[key]
            assert st["by_lds"] + st["by_long"] + st["skipped"] == len(reads), st
            for n, read in enumerate(reads):
                want = MR.map_read(X, read, P, second)
                assert got[n] == want, (case["name"], n, got[n], want)
            return got

        got = MR.run_case(CASES, case, mapper)
        want = MR.expected_outputs(CASES, case)
        assert sorted(got) == sorted(want)
        for f in want:
            assert got[f] == want[f], (case["name"], f)
        res[case["name"]] = stats
    return res


def large():
    """200 k reads of 250 bases on 2.5 Mb of contigs: a 5 000-read sample against the restatement, two batch sizes"""
    from dbg_assembly_amd import capi
    from oracle import oracle_py as O
    n_reads, k, s = 200000, 31, 5
    cb, co = O.synth_reads(O.synth_params(3000000, 5000, sub_rate=0.0, n_rate=0.0, cfg=7), 0, 500)
    contigs = [cb[int(co[i]):int(co[i + 1])].tobytes() for i in range(500)]
    bases, offsets = O.synth_reads(O.synth_params(3000000, 250, sub_rate=0.01, n_rate=0.001, cfg=7), 0, n_reads)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    P = MR.Params(k=k, s=s, l=125, r=250, i=0.97, fmt=1)
    with capi.Mapper(k=k, s=s, r=250, identity=0.97, second_alignment=True) as m:
        m.set_contigs(contigs)
        whole = m.map(bases, offsets)
        st = m.batch_stats()
        parts = []
        step = 37777
        for a in range(0, n_reads, step):
            b = min(n_reads, a + step)
            o = offsets[a:b + 1]
            parts.append(m.map(bases[int(o[0]):int(o[-1])], o - o[0]))
        m.set_ramp(64)
        flat = m.map(bases, offsets)
    assert np.array_equal(np.concatenate(parts), whole), "hits depend on the batch size"
    assert np.array_equal(flat, whole), "hits depend on the ramp of the seed scan"
    X = MR.Index(contigs, k)
    rng = np.random.default_rng(5)
    got = to_hits(whole)
    diffs = 0
    for i in sorted(rng.choice(n_reads, 5000, replace=False)):
        read = bases[int(offsets[i]):int(offsets[i + 1])].tobytes()
        diffs += got[i] != MR.map_read(X, read, P, True)
    assert diffs == 0, diffs
    mapped = int((whole["contig"][:, 0] != -1).sum())
    return {"reads": n_reads, "mapped": mapped, "second": int((whole["contig"][:, 1] != -1).sum()),
            "windows_per_read": st["windows_probed"] / n_reads, "ms_map": st["ms_map"]}


if __name__ == "__main__":
    print(json.dumps({"capi_goldens": capi_goldens, "large": large}[sys.argv[1]]()))
