"""CPU: the PAIR stage without a device.  The numpy restatement of the split (tests/pair_restatement.py) against a plain loop and
against the files the real reference wrote with -j 1 (tests/golden/pair_cases, made by tests/golden/make_pair_golden.py); the binding
against the header; and the two refusals of correct_error_reads -j 1 that come before any device work."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_restatement as PR  # noqa: E402
from dbg_assembly_amd import capi  # noqa: E402

EXE = os.path.join(ROOT, "dbg_assembly_amd", "bin", "correct_error_reads")


def loop_split(reads1, reads2):
    """merge_two_corr_files on lists of bytes -> ([(id, read)] of PAIR, of SINGLE)"""
    pair, single = [], []
    for i, (a, b) in enumerate(zip(reads1, reads2)):
        if a and b:
            pair += [(2 * i, a), (2 * i + 1, b)]
        else:
            if a:
                single.append((2 * i, a))
            if b:
                single.append((2 * i + 1, b))
    return pair, single


def test_restatement_equals_the_plain_loop_on_planes_offsets_ids_and_counters():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 65, 300):
        for with_qual in (False, True):
            lens = [np.where(rng.random(n) < 0.3, 0, rng.integers(1, 40, n)) for _ in range(2)]
            reads = [[rng.integers(65, 91, int(x), dtype=np.uint8).tobytes() for x in ls] for ls in lens]
            quals = [[rng.integers(33, 64, int(x), dtype=np.uint8).tobytes() for x in ls] for ls in lens]
            (b1, o1), (b2, o2) = PR.pack(reads[0]), PR.pack(reads[1])
            q1, q2 = (PR.pack(quals[0])[0], PR.pack(quals[1])[0]) if with_qual else (None, None)
            out, counters, max_len = PR.split(b1, o1, b2, o2, q1, q2)
            for which, want, want_q in zip((PR.PAIRED, PR.SINGLE), loop_split(*reads), loop_split(*quals)):
                bases, qplane, off, ids = out[which]
                assert ids.tolist() == [i for i, _ in want]
                assert PR.as_lines(bases, off) == [r for _, r in want]
                assert bases.size % 16 == 0 and bases.size - int(off[-1]) < 16 and not bases[int(off[-1]):].any()
                assert (qplane is None) == (not with_qual)
                if with_qual:
                    assert PR.as_lines(qplane, off) == [r for _, r in want_q] and not qplane[int(off[-1]):].any()
            pair, single = loop_split(*reads)
            assert counters == {"pair_reads": len(pair), "pair_bases": sum(len(r) for _, r in pair), "single_reads": len(single),
                                "single_bases": sum(len(r) for _, r in single)}
            assert max_len == max([len(r) for rs in reads for r in rs], default=0)


def test_restatement_takes_offsets_that_do_not_start_at_0():
    b = np.arange(100, dtype=np.uint8)
    out, counters, _ = PR.split(b, np.array([3, 3, 10], dtype=np.uint64), b, np.array([50, 57, 60], dtype=np.uint64))
    assert out[PR.PAIRED][0][:10].tolist() == list(range(3, 10)) + [57, 58, 59] and out[PR.PAIRED][3].tolist() == [2, 3]
    assert out[PR.SINGLE][0][:7].tolist() == list(range(50, 57)) and out[PR.SINGLE][3].tolist() == [1]
    assert counters == {"pair_reads": 2, "pair_bases": 10, "single_reads": 1, "single_bases": 7}


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_restatement_reproduces_the_reference_files_byte_for_byte(name):
    """every read is corrected independently of its place in its file, so the reference's output for mate file 2 (the records of mate
    file 1 rotated by one, which the reference removes after the merge) is the committed per-file golden rotated by one"""
    recs1 = PR.fa_records(os.path.join(PR.CORRECT, PR.CASES[name][0] + ".correct.fa.gz"))
    recs2 = PR.rotate(recs1)
    assert len(recs1) == 412 and PR.classes(recs1, recs2) == PR.CASES[name][2]
    pair, single, stat = PR.merged_text(recs1, recs2)
    assert pair == gzip.open(os.path.join(PR.GOLDEN, name + ".pair.fa.gz"), "rb").read()
    assert single == gzip.open(os.path.join(PR.GOLDEN, name + ".single.fa.gz"), "rb").read()
    assert stat == open(os.path.join(PR.GOLDEN, name + ".pair.single.stat"), "rb").read()


def test_goldens_are_small_data_files():
    names = sorted(os.listdir(PR.GOLDEN))
    assert names == sorted(n + ext for n in PR.CASES for ext in (".pair.fa.gz", ".single.fa.gz", ".pair.single.stat"))
    assert all(os.path.getsize(os.path.join(PR.GOLDEN, n)) < 64 << 10 for n in names)


# ---- the binding against the header ------------------------------------------------------------------------------------------------------
CTYPES = {"int": C.c_int, "uint64_t": C.c_uint64}
NEW = ("dbgk_pair_create", "dbgk_pair_destroy", "dbgk_pair_split_from", "dbgk_pair_split_device", "dbgk_pair_results", "dbgk_pair_device",
       "dbgk_push_pairs", "dbgk_map_reads_device")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dbgk.h")).read(), flags=re.S)


def declared(name):
    """the parameter types of a prototype of the header as the binding's ctypes: a value keeps its type, dbgk_pair_info * and the
    out-pointers of dbgk_pair_device are typed pointers, every other pointer is a void pointer"""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, name
    out = []
    for param in m.group(1).split(","):
        param = " ".join(param.split())
        stars = param.count("*")
        base = param.replace("const ", "").replace("*", " ").split()[0]
        if stars == 0:
            out.append(CTYPES[base])
        elif base == "dbgk_pair_info":
            out.append(C.POINTER(capi.PairInfo))
        elif stars == 2:
            out.append(C.POINTER(C.c_void_p))
        elif base == "uint64_t" and name == "dbgk_pair_device":
            out.append(C.POINTER(C.c_uint64))
        else:
            out.append(C.c_void_p)
    return out


def test_binding_declares_the_new_calls_with_the_signatures_of_the_header():
    table = {s[0]: s for s in capi.SYMBOLS}
    for name in NEW:
        assert name in table, name
        assert table[name][1] is C.c_int
        assert table[name][2] == declared(name), (name, table[name][2], declared(name))
    L = capi.lib()
    for name in NEW:
        assert hasattr(L, name)


def test_abi_is_still_7_and_the_info_struct_has_the_layout_of_the_header():
    assert int(re.search(r"#define\s+DBGK_ABI_VERSION\s+(\d+)", header()).group(1)) == 7 and capi.lib().dbgk_abi_version() == 7
    body = re.search(r"typedef struct dbgk_pair_info \{(.*?)\} dbgk_pair_info;", header(), flags=re.S).group(1)
    fields = [(n.strip(), t) for t, names in re.findall(r"(uint64_t|double)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [(n, "uint64_t" if t is C.c_uint64 else "double") for n, t in capi.PairInfo._fields_]
    assert C.sizeof(capi.PairInfo) == 64
    assert (capi.PAIR_PAIRED, capi.PAIR_SINGLE) == tuple(int(re.search(r"#define\s+DBGK_PAIR_%s\s+(\d+)" % w, header()).group(1))
                                                         for w in ("PAIRED", "SINGLE"))


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    assert L.dbgk_pair_create(0, None) == capi.ERR_ARG
    h = C.c_void_p()
    assert L.dbgk_pair_create(-1, C.byref(h)) == capi.ERR_ARG and not h
    info = capi.PairInfo()
    assert L.dbgk_pair_split_from(None, None, None, None, None, None, None, 0, C.byref(info)) == capi.ERR_ARG
    assert L.dbgk_pair_results(None, 0, None, None, None, None) == capi.ERR_ARG
    assert L.dbgk_push_pairs(None, None, 0) == capi.ERR_ARG
    assert L.dbgk_map_reads_device(None, None, None, 0, 0, 0, None) == capi.ERR_ARG


# ---- correct_error_reads -j 1 ------------------------------------------------------------------------------------------------------------
def test_j1_with_an_odd_number_of_files_is_refused_before_the_device_is_touched(tmp_path):
    """three files, none of which exists, and a table that does not exist: the program says why it stops and exits 1 without having
    tried to open any of them -- the check stands in front of dbgk_corr_create, so this holds with and without a GPU"""
    lib = tmp_path / "reads.lib"
    lib.write_text("".join("%s\n" % (tmp_path / ("r%d.fq" % i)) for i in range(3)))
    r = subprocess.run([EXE, "-k", "13", "-j", "1", str(tmp_path / "none.cz"), str(lib)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "-j 1 needs the read1 and read2 files in pairs" in r.stderr and "lists 3 files" in r.stderr
    assert "dbgk_corr_create" not in r.stderr and "no usable HIP device" not in r.stderr and "Fail to open" not in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["reads.lib"]
    src = open(os.path.join(ROOT, "dbg_assembly_amd", "host", "correct_error_reads.cpp")).read()
    assert src.index("lists \" << reads_files.size()") < src.index("dbgk_corr_create(&p")
    assert "not supported by this build" not in src


@pytest.mark.parametrize("content", [None, "", " \n\t\n"])
def test_j1_with_a_list_of_no_files_is_refused_before_the_device_is_touched(tmp_path, content):
    """a list that cannot be read, is empty or holds blank lines only names no pair to merge"""
    lib = tmp_path / "reads.lib"
    if content is not None:
        lib.write_text(content)
    r = subprocess.run([EXE, "-k", "13", "-j", "1", str(tmp_path / "none.cz"), str(lib)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-j 1 needs the read1 and read2 files in pairs" in r.stderr and "lists 0 files" in r.stderr
    assert "dbgk_corr_create" not in r.stderr and "no usable HIP device" not in r.stderr and "Fail to open" not in r.stderr
    # without -j 1 the same list is no error of this check: the program goes on to the device and the table, as before
    r = subprocess.run([EXE, "-k", "13", str(tmp_path / "none.cz"), str(lib)], capture_output=True, text=True, timeout=60)
    assert "-j 1" not in r.stderr


def test_usage_text_is_unchanged():
    r = subprocess.run([EXE], capture_output=True, timeout=60)
    assert r.stdout == open(os.path.join(ROOT, "tests", "golden", "correct_usage.txt"), "rb").read()
