"""CPU: tests/parse_restatement.py, the plain statement of the PARSE stage's rule, anchored to code that is already pinned -- the
two file readers of host/reads_io.h through tests/reads_io_test.cpp (sequences, on every crafted text of tests/parse_cases.py) and
the cleaners' record loop RecordBatch::fill through tests/parse_fill_test.cpp (headers, reads and qualities of the CLEAN golden
inputs) -- and its own chunking property: a text fed in two chunks with the carry-over gives the records of the whole text."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parse_cases as PC  # noqa: E402
import parse_restatement as PR  # noqa: E402
from test_reads_io import expected_records  # noqa: E402

HOST = os.path.join(ROOT, "dbg_assembly_amd", "host")
CASES = PC.cases()


@pytest.fixture(scope="module")
def reads_io_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("parse_readsio") / "reads_io_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + HOST, os.path.join(ROOT, "tests", "reads_io_test.cpp"), "-o", out, "-lz", "-lpthread"], check=True)
    return out


@pytest.fixture(scope="module")
def fill_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("parse_fill") / "parse_fill_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "parse_fill_test.cpp"),
                    "-o", out, "-lz"], check=True)
    return out


def counted_lines(out):
    """lines "<len>\\t<text>" whose text may hold anything but a newline"""
    got = []
    for line in out.split(b"\n")[:-1]:
        n, text = line.split(b"\t", 1)
        assert int(n) == len(text)
        got.append(text)
    return got


def test_sequences_equal_both_host_readers_on_every_crafted_text(reads_io_exe, tmp_path):
    path = str(tmp_path / "in.txt")
    for name, (fmt, text) in CASES.items():
        with open(path, "wb") as f:
            f.write(text)
        mine = [seq for _, seq, _ in PR.parse(text, fmt)["records"]]
        assert mine == expected_records(text, fmt), name
        for threads in (0, 3):
            r = subprocess.run([reads_io_exe, path, str(fmt), str(threads)], capture_output=True, check=True)
            assert counted_lines(r.stdout) == mine, (name, threads)


@pytest.mark.parametrize("name", ["reads", "mixed", "phred64", "norecords"])
def test_records_equal_the_cleaners_record_loop_on_the_golden_inputs(fill_exe, name):
    path = os.path.join(PC.CLEAN, name + ".fq")
    text = open(path, "rb").read()
    r = subprocess.run([fill_exe, path], capture_output=True, check=True)
    tail = r.stdout.rstrip(b"\n").rsplit(b"\n", 1)[-1]
    lines = counted_lines(r.stdout[:len(r.stdout) - len(tail) - 1])
    want = [tuple(lines[i:i + 3]) for i in range(0, len(lines), 3)]
    got = PR.parse(text, 1, with_quals=False)
    assert got["records"] == want
    assert [int(x) for x in tail.split(b"\t")] == [got["info"]["n_records"], got["info"]["n_bases"]]
    assert (name == "norecords") == (not want)
    # with a quality plane: clean_lowqual's emptying of a record whose two strings differ in length (host/clean_lowqual.cpp:75-79)
    q = PR.parse(text, 1, with_quals=True)
    kept = [(s, ql) if len(s) == len(ql) else (b"", b"") for _, s, ql in want]
    nb = int(q["offsets"][-1])
    assert q["bases"][:nb].tobytes() == b"".join(s for s, _ in kept) and q["quals"][:nb].tobytes() == b"".join(ql for _, ql in kept)
    assert np.array_equal(np.diff(q["offsets"].astype(np.int64)), [len(s) for s, _ in kept])
    assert q["info"]["mismatched"] == sum(1 for _, s, ql in want if len(s) != len(ql))


def test_the_records_describe_the_text_and_the_planes():
    for name, (fmt, text) in CASES.items():
        for with_quals in ((False, True) if fmt == 1 else (False,)):
            got = PR.parse(text, fmt, with_quals)
            off, nb = got["offsets"].astype(np.int64), int(got["offsets"][-1])
            assert got["bases"].size == -(-nb // 16) * 16 and not got["bases"][nb:].any(), name
            assert got["info"]["consumed"] == len(text) and got["info"]["n_lines"] == len(PR.lines_of(text)), name
            for i, (r, (head, seq, qual)) in enumerate(zip(got["recs"], got["records"])):
                assert text[r["head_pos"]:r["head_pos"] + r["head_len"]] == head and text[r["seq_pos"]:r["seq_pos"] + r["seq_len"]] == seq, name
                assert text[r["qual_pos"]:r["qual_pos"] + r["qual_len"]] == qual, name
                emptied = with_quals and len(seq) != len(qual)
                assert got["bases"][off[i]:off[i + 1]].tobytes() == (b"" if emptied else seq), name
                if with_quals:
                    assert got["quals"][off[i]:off[i + 1]].tobytes() == (b"" if emptied else qual), name


def every_split(text):
    if len(text) <= 400:
        return range(1, len(text) + 1)
    return sorted(set(list(range(1, 130)) + list(range(PC.T - 40, PC.T + 40)) + list(range(len(text) - 130, len(text) + 1))))


def test_two_chunks_with_the_carry_over_give_the_records_of_the_whole_text():
    for name, (fmt, text) in CASES.items():
        if len(text) > 3 * PC.T:
            continue
        for with_quals in ((False, True) if fmt == 1 else (False,)):
            whole = PR.parse(text, fmt, with_quals)
            for cut in every_split(text):
                first = PR.parse(text[:cut], fmt, with_quals, last=False)   # [0, cut), then the carry and the rest
                assert first["info"]["consumed"] <= cut
                rest = text[first["info"]["consumed"]:]
                parts = [(text[:cut], first), (rest, PR.parse(rest, fmt, with_quals, last=True))]
                records, sums = PR.joined(parts)
                assert records == whole["records"], (name, cut)
                assert sums == {f: whole["info"][f] for f in PR.SUMMED}, (name, cut)
                assert sum(got["info"]["consumed"] for _, got in parts) == len(text), (name, cut)


def test_a_stream_of_small_windows_equals_the_whole_text():
    for name in ("junk_empty_lines_empty_header", "quality_starts_with_at", "lengths_0_100", "fasta_400_reads", "crlf"):
        fmt, text = CASES[name]
        whole = PR.parse(text, fmt, fmt == 1)
        for window in ((1, 7, 64, 1000) if len(text) < 2000 else (64, 1000)):
            parts = PR.stream(text, fmt, window, fmt == 1)
            records, sums = PR.joined(parts)
            assert records == whole["records"] and sums == {f: whole["info"][f] for f in PR.SUMMED}, (name, window)
            assert max(got["info"]["max_len"] for _, got in parts) == whole["info"]["max_len"]
        assert PR.stream(text, fmt, 3, fmt == 1)[0][1]["info"]["consumed"] == 0   # smaller than one record
