"""CPU: the contig stage's first pass for tables of 32-byte nodes (dbgk_wide_export_host_table_links and the communicator's form):
the two symbols and their binding, their argument checks, the host-side patch for the nodes that live outside the device table
(tests/wide_links_patch_test.cpp, a program of its own built with the address and undefined-behaviour sanitizers), and the inputs
the GPU tests rely on.  PARITY UNPINNED above k = 32."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contig_restatement as R  # noqa: E402
import wide_contig_restatement as W  # noqa: E402
import wide_links_gpu_steps as S  # noqa: E402
from dbg_assembly_amd import capi  # noqa: E402

NAMES = ("dbgk_wide_export_host_table_links", "dbgk_comm_wide_export_host_table_links")
# (handle or communicator, host_size, array, nul_flag, kmer_freq_cutoff, klink, del_flag, tip_nodes, tip_capacity, n_tips, branch_nodes,
#  branch_capacity, n_branches, stats)
ARGS = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
        C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]


def test_the_library_exports_both_calls_and_the_binding_has_their_arguments():
    """fails on a build without the feature: neither symbol exists"""
    L = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    for name in NAMES:
        assert hasattr(L, name), "libdbgk.so does not export %s" % name
        assert name in bound and bound[name][1] is C.c_int and list(bound[name][2]) == ARGS, name
    assert callable(capi.Graph.wide_export_host_table_links) and callable(capi.Comm.wide_export_host_table_links)


def test_a_null_handle_or_communicator_is_an_argument_error():
    import numpy as np
    L = capi.lib()
    a, f, kl, d = np.zeros(3, capi.NODE32_DTYPE), np.zeros(1, np.uint8), np.zeros(3, np.uint16), np.zeros(1, np.uint8)
    nt, nb = C.c_uint64(), C.c_uint64()
    for name in NAMES:
        rc = getattr(L, name)(None, 3, a.ctypes.data, f.ctypes.data, 2, kl.ctypes.data, d.ctypes.data, None, 0, C.byref(nt), None, 0, C.byref(nb), None)
        assert rc == capi.ERR_ARG, (name, rc)


def test_patch_for_the_nodes_placed_on_the_host_under_the_sanitizers(tmp_path):
    """the HIP-free patch header, compiled with the system C++ compiler and -fsanitize=address,undefined into a program with its own
    main and run as such, in the environment as it is"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no system C++ compiler"
    exe = tmp_path / "wide_links_patch_test"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts whatever else the process loads
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dbg_assembly_amd", "csrc"),
                    os.path.join(ROOT, "tests", "wide_links_patch_test.cpp"), "-o", str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("cases ok") and int(r.stdout.split()[0]) >= 20


@pytest.fixture(scope="module")
def placed_tables():
    """the reads of the `placed` GPU step and of the command-line tests, laid out in Python at the table size of `-i 0.00003`, after
    first_pass at every cutoff tried: {(k, cutoff): (table, tips, branches)}"""
    out = {}
    for k in S.KS:
        seqs = [(r, 1) for r in S.placed_reads(k)]
        for cutoff in S.CUTOFFS:
            t = W.build_table(seqs, k, S.PLACED_SIZE)
            tips, branches, stat, _ = R.first_pass(t, R.Options(D=cutoff))
            out[(k, cutoff)] = (t, tips, branches, stat)
    return out


def test_the_crafted_reads_put_placed_nodes_inside_both_lists(placed_tables):
    """what the GPU test relies on (and asserts again on the table it gets, whose slots are the program's): tips and branches with a
    zero low word, not only at the ends of their lists, lists over more than one block of 4096 slots; besides: a deleted node with a
    zero low word at cutoff 2, the key-0 node a branch and linear at cutoff 5, counters at 255, a side with four links"""
    S.placed_conditions({key: v[:3] for key, v in placed_tables.items()})
    for (k, cutoff), (t, tips, branches, stat) in placed_tables.items():
        assert all(len(r) <= 150 for r in S.placed_reads(k))
        zero_low = [i for i in range(t.size) if t.filled[i] and t.kmer[i] & W.M64 == 0]
        assert len(zero_low) == 4 and sum(1 for i in zero_low if t.kmer[i] == 0) == 1
        slot0 = next(i for i in zero_low if t.kmer[i] == 0)
        assert (slot0 in branches) == (cutoff < 5) and t.linear[slot0] == (cutoff == 5)
        if cutoff == 2:
            assert any(t.deleted[i] for i in zero_low)
        assert stat[255] > 0
        assert any(t.filled[i] and (t.l_num[i] == 3 or t.r_num[i] == 3) and
                   4 in (sum(1 for j in range(4) if R.depth_of(t.l_link[i], j) > cutoff), sum(1 for j in range(4) if R.depth_of(t.r_link[i], j) > cutoff))
                   for i in range(t.size)) or cutoff == 5
