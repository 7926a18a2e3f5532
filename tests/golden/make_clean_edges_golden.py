"""Writes tests/golden/clean_edges: the crafted scenarios of tests/clean_edge_cases.py as FASTQ and contaminant FASTA, and what the
REFERENCE's own clean_adapter and clean_lowqual make of them.

    python tests/golden/make_clean_edges_golden.py <directory of the reference>

The two programs are taken ready built from <reference>/clean_illumina/, as make_clean_golden.py takes them.  Nothing of the
reference but data is stored: per pinned scenario the inputs (<name>.fq.gz, <name>.fa), <name>/out.gz and <name>/out.stat, and
cases.json with the command lines.  A scenario with `_unpinned` in its name is not written: the reference indexes outside its
alphabet[] / Qual2Err with such bytes.  Before anything is stored the script asserts that the restatement reproduces each output.
No test runs this script; the tests read what it left.
"""
import gzip
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clean_edge_cases as E  # noqa: E402
import clean_restatement as CR  # noqa: E402

OUT = os.path.join(HERE, "clean_edges")
LARGEST_BEFORE = 486909      # bytes of the largest golden the repository had before this set


def write_inputs(scn, directory):
    with gzip.GzipFile(os.path.join(directory, scn.name + ".fq.gz"), "wb", mtime=0) as f:
        f.write(E.fastq(scn))
    if isinstance(scn, E.AdapterScenario):
        open(os.path.join(directory, scn.name + ".fa"), "wb").write(E.fasta(scn))


def main():
    ref = os.path.join(sys.argv[1], "clean_illumina")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    cases = []
    for scn in E.scenarios():
        if not E.pinned(scn):
            continue
        case = E.case_of(scn)
        write_inputs(scn, OUT)
        os.makedirs(os.path.join(OUT, scn.name))
        subprocess.run([os.path.join(ref, case["program"])] + case["args"] + [case["input"], os.path.join(scn.name, "out.gz"),
                                                                             os.path.join(scn.name, "out.stat")],
                       cwd=OUT, check=True, capture_output=True, timeout=600)
        want, got = CR.expected_outputs(OUT, case), CR.run_case(OUT, case)
        assert got["out"] == want["out"] and got["stat"] == want["stat"], "the restatement differs from the reference: " + scn.name
        for a, b in zip(got["numbers"], E.restated(scn.name)):
            assert tuple(a) == tuple(b), scn.name
        cases.append(case)
    json.dump(cases, open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    sizes = {os.path.join(dp, f): os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(OUT) for f in fs}
    assert max(sizes.values()) < LARGEST_BEFORE, max(sizes, key=sizes.get)
    print("wrote %d files, %d bytes in all, largest %d bytes" % (len(sizes), sum(sizes.values()), max(sizes.values())))


if __name__ == "__main__":
    main()
