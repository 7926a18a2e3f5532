"""GPU steps of tests/test_l1_forms_gpu.py, each run in a child process of its own under a time limit:
    python tests/l1_forms_gpu_steps.py <step>
A step creates ONE handle -- an engine, a k, a table size -- and runs the cases of tests/l1_form_cases.py that belong to it, with
reset() between them: the reads through the case's entry point under the case's hooks, finalize, then
    Graph.l1_forms() == the case's launches (rows and order)                                the row ran under its own name
    graph: (total_reads, total_kmers, count), the key-0 node's link counters, other_bytes, export_sorted() against oracle.build_graph
    KFREQ: the whole 4^k-byte table against the counting restatement (oracle.kfreq_expected_counts), count, stored k-mers
    WIDE:  (total_reads, total_kmers, count), other_bytes, digest(), wide_export_sorted() against oracle.wide_build
Tables of 2^31 slots and more: digest() against the oracle's for every row, the full export once per handle.
Prints one JSON line; exits non-zero on the first mismatch, naming the row.

STEPS: step -> (seconds measured on an MI355X, time limit = five times that, at least 60 s)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import l1_form_cases as LC  # noqa: E402
from helpers import hooks_value  # noqa: E402

STEPS = {
    # tier A: small tables
    "graph_k31_w0_reg": (2.3, 60), "graph_k31_w0_uniform": (2.3, 60), "graph_k31_w0_other": (2.3, 60), "graph_k16_w0_all": (2.6, 60),
    "kfreq_k13_w0_uniform": (3.8, 60), "kfreq_k13_w0_other": (3.6, 60), "wide_k63_w0_all": (2.3, 60),
    # tier B: tables of 2^31 and of 2^32 slots and more
    "graph_k31_w1_reg": (3.6, 60), "graph_k31_w1_uniform": (3.1, 60), "graph_k31_w1_other": (2.6, 60), "graph_k16_w1_all": (2.7, 60),
    "wide_k63_w1_all": (3.2, 60),
    "graph_k31_w2_reg": (3.0, 60), "graph_k31_w2_uniform": (2.6, 60), "graph_k31_w2_other": (2.2, 60), "graph_k16_w2_all": (3.7, 60),
    "wide_k63_w2_all": (4.3, 60),
}


def step_of(case):
    """the handle a case runs on, and -- where a handle has more than about a dozen rows -- the part of its rows"""
    part = "all"
    if (case.engine, case.k) in (("graph", 31), ("kfreq", 13)):
        part = "reg" if " reg=1 " in case.row else "uniform" if case.row.startswith("family=uniform ") else "other"
    return "%s_k%d_w%d_%s" % (case.engine, case.k, case.width, part)


def cases_of(step):
    return [c for _, c in sorted(LC.cases().items()) if step_of(c) == step and c.row not in LC.UNSELECTABLE]


def create(capi, case):
    if case.engine == "kfreq":
        return capi.Graph(k=case.k, table_slots=0, engine=capi.ENGINE_KFREQ, max_read_len=case.max_read_len, expected_kmers=LC.EXPECTED_KMERS)
    size = capi.find_next_prime_ref(LC.SLOTS[case.width])
    if case.engine == "wide":
        g = capi.Graph(k=case.k, table_slots=size, max_read_len=case.max_read_len, engine=capi.ENGINE_WIDE, expected_kmers=LC.EXPECTED_KMERS,
                       n_passes=1 if case.passes > 1 else 0)
        assert g.wide_pass_info()[0] == case.passes, g.wide_pass_info()
        return g
    return capi.Graph(k=case.k, table_slots=size, max_read_len=case.max_read_len, engine=capi.ENGINE_PARTITION, expected_kmers=LC.EXPECTED_KMERS)


def push(capi, g, case, bases, offsets):
    if case.entry == "push_reads":
        g.push_reads(bases, offsets)
        return
    words, other = capi.pack_bases(bases)
    if case.entry == "push_reads_packed":
        g.push_reads_packed(words, offsets, other)
    else:
        assert case.entry == "push_reads_packed_uniform"
        g.push_reads_packed_uniform(words, len(offsets) - 1, int(offsets[1]), other)


def run_case(capi, oracle, g, case, full_export):
    reads = LC.reads(case)
    bases, offsets = oracle.pack_reads(reads)
    hooks = hooks_value(None, **case.hooks)      # (read once per batch)
    if hooks:
        os.environ["DBGK_TEST_HOOKS"] = hooks
    else:
        os.environ.pop("DBGK_TEST_HOOKS", None)
    for p in range(case.passes):
        if case.passes > 1:
            g.wide_begin_pass(p)
        push(capi, g, case, bases, offsets)
        if case.passes > 1:
            g.wide_end_pass()
    st = g.finalize()
    forms = g.l1_forms()
    assert forms == case.launches and g.l1_launches == len(forms), ("forms", case.row, forms, case.launches)
    other = oracle.count_other_bytes(bases)
    assert other == 1 and int(st.other_bytes) == other, ("other_bytes", case.row, int(st.other_bytes))
    if case.engine == "kfreq":
        want = oracle.kfreq_expected_counts([(bases, offsets)], case.k, case.max_read_len)
        got = g.kfreq_counts()
        assert np.array_equal(got, want), ("counts", case.row, int((got != want).sum()))
        windows = sum(max(0, min(len(r), case.max_read_len) - case.k + 1) for r in reads)
        assert (int(st.total_reads), int(st.stored_kmers), int(st.count)) == (len(reads), windows, int((want > 0).sum())), ("stats", case.row)
    elif case.engine == "wide":
        want, total = oracle.wide_build(bases, offsets, case.k, case.max_read_len)
        assert (int(st.total_reads), int(st.total_kmers), int(st.count)) == (len(reads), total, len(want)), ("stats", case.row)
        assert g.digest() == oracle.wide_digest(want), ("digest", case.row)
        if full_export:
            assert np.array_equal(g.wide_export_sorted(), want), ("nodes", case.row)
    else:
        ref = oracle.build_graph(files_mem=[(bases, offsets)], k=case.k, max_read_len=case.max_read_len, init_hash_size=0.001, threads=1)
        want = ref.nodes.astype(capi.NODE_DTYPE)
        assert int(want[0]["kmer"]) == 0 and (int(want[0]["l_link"]) or int(want[0]["r_link"])), "the reads have no key-0 node"
        assert (int(st.total_reads), int(st.total_kmers), int(st.count)) == (ref.total_reads, ref.total_kmers, ref.count), ("stats", case.row)
        assert (int(st.polyA_l_link), int(st.polyA_r_link)) == (int(want[0]["l_link"]), int(want[0]["r_link"])), ("key 0", case.row)
        assert g.digest() == oracle.nodes_digest(ref.nodes), ("digest", case.row)
        if full_export:
            assert np.array_equal(g.export_sorted(), want), ("nodes", case.row)


def run_step(step):
    from dbg_assembly_amd import capi
    from oracle import oracle_py as oracle
    cases = cases_of(step)
    assert cases, step
    t0 = time.time()
    with create(capi, cases[0]) as g:
        created = time.time() - t0
        for i, case in enumerate(cases):
            if i:
                g.reset()
                assert g.l1_forms() == [], "reset() keeps the launches of the batch before"
            run_case(capi, oracle, g, case, full_export=case.width == 0 or i == 0)
    return {"step": step, "rows": len(cases), "create_s": round(created, 2), "seconds": round(time.time() - t0, 2)}


if __name__ == "__main__":
    print(json.dumps(run_step(sys.argv[1])))
