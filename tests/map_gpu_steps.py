"""GPU steps of tests/test_map_gpu.py, each run in a child process of its own under a time limit:
    python tests/map_gpu_steps.py capi_goldens | large | edges
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


def edges():
    """the crafted scenarios of tests/map_edge_cases.py at the first chunks 1, 4 and 64 of the seed scan: all eight fields of
    both hits equal the restatement's, the counters equal the census of lengths; one batch wide enough for the grid-stride
    loop; the reference-written goldens of the scenarios through capi.Mapper"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count   # torch's HIP runtime first, as tests/conftest.py has it
    from dbg_assembly_amd import capi
    import map_edge_cases as E
    from test_map_edges_cpu import EDGE_CASES, edge_expected, edge_golden_cases
    cats, stats = {}, {"by_lds": 0, "by_long": 0, "skipped": 0}

    def run(m, scn, idx, want):
        reads = [scn.reads[n] for n in idx]
        got = to_hits(m.map_sequences(reads))
        st = m.batch_stats()
        assert {key: st[key] for key in stats} == E.census(scn, reads), (scn.name, st)
        for n, g, w in zip(idx, got, want):
            assert g == w, (scn.name, n, scn.expect[n], g, w)
        for key in stats:
            stats[key] += st[key]
        return got

    for scn in E.scenarios():
        X, hits = E.restated(scn.name)
        with capi.Mapper(k=scn.k, s=scn.s, r=scn.r, identity=scn.identity, second_alignment=scn.second) as m:
            m.set_contigs(scn.contigs)
            per_ramp = []
            for ramp in E.RAMPS:
                m.set_ramp(ramp)
                per_ramp.append([run(m, scn, idx, [hits[n] for n in idx]) for idx in E.batches(scn)])
            assert per_ramp[0] == per_ramp[1] == per_ramp[2], (scn.name, "hits depend on the ramp of the seed scan")
        for e in scn.expect:
            cats[e["cat"]] = cats.get(e["cat"], 0) + len(E.RAMPS)
    # a partly filled last workgroup behind a full grid of 32 workgroups per CU, four reads each
    scn, idx = E.grid_reads(4 * 32 * n_cu + 5)
    X, hits = E.restated(scn.name)
    with capi.Mapper(k=scn.k, s=scn.s, r=scn.r, identity=scn.identity, second_alignment=scn.second) as m:
        m.set_contigs(scn.contigs)
        run(m, scn, idx, [hits[n] for n in idx])
    cats["grid"] = len(idx)
    golden = 0
    for case in edge_golden_cases():
        def mapper(X, reads, P, second):
            with capi.Mapper(k=P.k, s=P.s, r=P.r, identity=P.i, second_alignment=second) as m:
                m.set_contigs(X.contigs)
                return to_hits(m.map_sequences(reads))

        got, want = MR.run_case(EDGE_CASES, case, mapper), edge_expected(case)
        assert sorted(got) == sorted(want)
        for f in want:
            assert got[f] == want[f], (case["name"], f)
        golden += 1
    return dict(categories=cats, ramps=list(E.RAMPS), golden_cases=golden, n_cu=n_cu, **stats)


if __name__ == "__main__":
    print(json.dumps({"capi_goldens": capi_goldens, "large": large, "edges": edges}[sys.argv[1]]()))
