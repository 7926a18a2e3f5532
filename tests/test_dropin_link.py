"""CPU: guards of the drop-in boundary.

1. The reference's UNCHANGED consumer -- DBG_contig/main.cpp, contig.cpp, global_aligning.cpp -- compiles
   against dbg_assembly_amd/host/{seqKmer,kmerSet,DBGgraph}.h and links with libdbgasm_host.so + libdbgk.so
   (same globals, struct layouts and function names).  build() makes it
   where the reference sources are present (oracle/Makefile, oracle/_ref/ref_consumer: the sources are reached
   through links, so that their `#include "kmerSet.h"` resolves to THIS build's headers; nothing of the reference
   is copied or stored).  contig.h needs boost/lexical_cast.hpp: oracle/standin/ holds a throw-away stand-in.
   This is a LINK / ABI guard, not a parity pin -- a build that needs a stand-in header pins nothing, and the
   consumer is only asked for its usage text.
2. The format of `<prefix>.contig.kmer.freq` that tests/test_gpu_cli.py asserts for the GPU build is the
   format of the file the reference's own test directory holds (contig.cpp:199-202: header, rows 1..255, row 0
   omitted; stored as tests/golden/Ecoli_corrected_reads.contig.kmer.freq).  Format only: the producer of that
   file's numbers (contig.cpp:119-181) cannot be compiled here, so the DepthStat restatement in oracle/ stays
   "parity unpinned".
"""
import os
import subprocess

import pytest

from helpers import GOLDEN, KMER_FREQ_HEADER, KMER_FREQ_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSUMER = os.path.join(ROOT, "oracle", "_ref", "ref_consumer")


def test_reference_consumer_compiles_and_links_against_the_host_layer():
    if not os.path.exists(CONSUMER):
        pytest.skip("oracle/_ref/ref_consumer not built (the reference sources were not present where build() ran)")
    exe = CONSUMER
    # every symbol the consumer takes from the graph stage is resolved by the host layer
    nm = subprocess.run(["nm", "-u", "-C", exe], check=True, capture_output=True, text=True).stdout
    for sym in ("build_debruijn_graph", "exist_kmerset", "get_next_kmer_depth", "get_rev_com_kbit", "memset_parallel", "reading_file_list"):
        assert sym in nm, sym   # undefined in the consumer = taken from libdbgasm_host.so
    nm_all = subprocess.run(["nm", "-C", exe], check=True, capture_output=True, text=True).stdout
    for sym in ("kset", "KmerHeadMaskVal", "KmerSize"):   # data: copy-relocated into the executable
        assert any(line.split()[-1] == sym for line in nm_all.splitlines() if line.split()), sym
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)   # the reference's own usage text, no GPU touched
    assert r.returncode == 0 and "debruijn_contig" in r.stdout and "-k <int>" in r.stdout


def test_kmer_freq_file_format_matches_the_reference_fixture():
    path = os.path.join(GOLDEN, "Ecoli_corrected_reads.contig.kmer.freq")
    rows = open(path).read().splitlines()
    assert rows[0] == KMER_FREQ_HEADER and len(rows) == 1 + KMER_FREQ_ROWS
    for i, row in enumerate(rows[1:], start=1):   # rows 1..255, DepthStat[0] is not written (contig.cpp:200)
        depth, times = row.split("\t")
        assert int(depth) == i and int(times) >= 0
