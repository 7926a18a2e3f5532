"""CPU: which level-1 kernel form a batch takes (dbg_assembly_amd/csrc/dbgk_l1_form.h: the lists of instantiations and l1_plan), through
a small stand-alone program (tests/l1_form_main.cpp) built with the HIP compiler, its host side under ASan + UBSan.  The program runs
alone: nothing is loaded into Python.

  the plans      of the shapes at which the decision changes: regular tiles and the rest, partly filled lanes, lane counts that are no
                 power of two, k < 17, many level-1 buckets, the three table widths, mixed lengths with and without the hooks, KFREQ
                 direct blocks, the WIDE record engine.  Every form of every plan must have a row in its family's list.
  the lists      74 / 12 / 6 / 6 / 6 / 6 rows, no two equal, and as many kernels of each family in the built library's code object.
  the cases      tests/l1_form_cases.py, which tests/test_l1_forms_gpu.py runs on the GPU: one case per row, and the plan of every case on
                 the facts of the handle the library creates for it and of its actual reads is the launch list the case expects.
"""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ROWS = {"uniform": 74, "prefix": 12, "flat-linear": 6, "flat": 6, "wide-flat": 6, "wide-uniform": 6}
KERNEL_OF = {"uniform": "k_extract_scatter_uniform", "prefix": "k_extract_scatter_prefix", "flat-linear": "k_extract_scatter_lin",
             "flat": "k_extract_scatter", "wide-flat": "k_wide_scatter_l1", "wide-uniform": "k_wide_scatter_l1_uniform"}
W_PIPE_PK_WORDS = 912   # kWPipePkWords (dbgk_wide_partition.h)

# a PARTITION graph handle: maxReadLen 250, a table below 2^31 slots with 144 level-1 buckets, no hooks
GRAPH = dict(part=1, kmer_size=31, max_read_len=250, n1=144, geom_size=144 << 20, size=144 << 20)


def equal_reads(n_reads, length, **more):
    return dict(n_reads=n_reads, n_bases=n_reads * length, uniform_len=length, len_max=length, has_long=0, **more)


def mixed_reads(lengths, **more):
    return dict(n_reads=len(lengths), n_bases=sum(lengths), uniform_len=0, len_max=max(lengths), has_long=0, **more)


MIXED = [150] * 275 + [60 + (89 * i) // 24 for i in range(25)]   # 25 of 300 reads cut to 60 .. 149 bases


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "the HIP compiler is needed (as for the build)"
    exe = str(tmp_path_factory.mktemp("l1_form") / "l1_form_main")
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dbg_assembly_amd", "csrc"),
           os.path.join(ROOT, "tests", "l1_form_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")   # (the HIP runtime's own start-up allocations are not this program's)
    return subprocess.run([exe] + args, capture_output=True, text=True, env=env)


def plan(exe, *facts, **more):
    """the launches of a batch: a list of dicts (the form's and the geometry's fields as integers, the family as text)"""
    merged = {}
    for f in facts + (more,):
        merged.update(f)
    res = run(exe, ["plan"] + ["%s=%d" % kv for kv in merged.items()])
    assert res.returncode == 0, (merged, res.stdout, res.stderr[-2000:])   # (1: a form without a row)
    lines = res.stdout.splitlines()
    head = dict(kv.split("=") for kv in lines[0].split()[1:])
    launches = []
    for line in lines[1:]:
        assert line.startswith("launch "), line
        d = dict(kv.split("=") for kv in line.split()[1:])
        launches.append({k: (v if k == "family" else int(v)) for k, v in d.items()})
    assert int(head["launches"]) == len(launches)
    return launches


def has(launch, **fields):
    return all(launch[k] == v for k, v in fields.items())


def test_equal_lengths_regular_tiles_and_the_rest(program):
    for packed in (1, 0):
        reg, rest = plan(program, GRAPH, equal_reads(300, 150, packed=packed))
        assert has(reg, family="uniform", wide_d=0, c=15, ragged=0, lin=0, reg=1, packed=packed, full=1, k17=1, dbg=0), reg
        assert has(reg, L=150, W=120, Q=8, lq=3, tile_blocks=1200, first_read=0, n_reads=256, tiles=2, n_lanes=2048), reg
        assert has(rest, family="uniform", wide_d=0, c=15, ragged=0, lin=0, reg=0, packed=0, k17=1, dbg=0), rest
        assert has(rest, Q=8, first_read=256, n_reads=44, n_lanes=352, tiles=1), rest
    # 256 reads: whole tiles only
    only, = plan(program, GRAPH, equal_reads(256, 150, packed=1))
    assert has(only, reg=1, n_reads=256, tiles=2), only
    # partly filled lanes: 121 windows = 7 * 16 + 9
    reg, rest = plan(program, GRAPH, equal_reads(300, 151, packed=1))
    assert has(reg, family="uniform", c=16, reg=1, full=0, k17=1, Q=8, tile_blocks=1208), reg
    assert has(rest, family="uniform", c=16, reg=0, k17=1, n_reads=44), rest


def test_equal_lengths_without_regular_tiles(program):
    one, = plan(program, GRAPH, equal_reads(300, 100, packed=1))        # five lanes per read: no power of two
    assert has(one, family="uniform", c=15, reg=0, ragged=0, lin=0, k17=1, Q=5, tile_blocks=0, n_reads=300), one
    one, = plan(program, GRAPH, equal_reads(300, 150, packed=1), kmer_size=16)
    assert has(one, family="uniform", c=15, reg=0, k17=0, Q=9, tile_blocks=0), one


def test_many_buckets_take_the_linear_form(program):
    one, = plan(program, GRAPH, equal_reads(300, 150, packed=1), n1=573)
    assert has(one, family="uniform", lin=1, c=12, Q=10, k17=1, reg=0, ragged=0, n_lanes=3000), one
    assert plan(program, GRAPH, equal_reads(300, 150, packed=1), n1=573, l1_linear=0) == plan(program, GRAPH, equal_reads(300, 150, packed=1))
    assert plan(program, GRAPH, equal_reads(300, 150, packed=1), l1_linear=1) == [one]
    # the threshold itself (tests/test_l1_tile_tail.py runs up to 257 buckets on the wave-per-bucket side of it)
    assert [plan(program, GRAPH, equal_reads(300, 150), n1=n)[-1]["lin"] for n in (320, 321)] == [0, 1]
    # reads too short for a uniform form, many buckets: the flat kernel's linear form, not the prefix form
    for has_long in (0, 1):
        one, = plan(program, GRAPH, equal_reads(300, 80), n1=573, has_long=has_long)
        assert has(one, family="flat-linear", has_dead=has_long, wide_d=0), one


def test_table_widths(program):
    for size, wide_d in ((1 << 31, 1), (1 << 32, 2), ((1 << 31) - 1, 0), ((1 << 32) - 1, 1)):
        at = dict(geom_size=size, size=size)
        assert [l["wide_d"] for l in plan(program, GRAPH, equal_reads(300, 150, packed=1), at)] == [wide_d, wide_d]
        narrow = plan(program, GRAPH, equal_reads(300, 150, packed=1))
        assert [dict(l, wide_d=0) for l in plan(program, GRAPH, equal_reads(300, 150, packed=1), at)] == narrow
        for facts in (dict(n1=573), dict(kmer_size=16)):
            one, = plan(program, GRAPH, equal_reads(300, 150), at, facts)
            assert one["wide_d"] == wide_d and dict(one, wide_d=0) == plan(program, GRAPH, equal_reads(300, 150), facts)[0]
        assert plan(program, GRAPH, mixed_reads(MIXED), at)[0]["wide_d"] == wide_d
        assert plan(program, GRAPH, equal_reads(300, 80), at, l1_prefix=0)[0]["wide_d"] == wide_d


def test_mixed_lengths(program):
    assert min(MIXED) == 60 and max(l for l in MIXED if l < 150) == 149 and sum(l < 150 for l in MIXED) == 25
    one, = plan(program, GRAPH, mixed_reads(MIXED))
    assert has(one, family="prefix", k17=1, c=15, wide_d=0, n_reads=300), one
    one, = plan(program, GRAPH, mixed_reads(MIXED), l1_prefix=0)
    assert has(one, family="uniform", ragged=1, k17=1, c=15, reg=0, lin=0, Q=8, n_lanes=2400), one
    for has_long in (0, 1):
        one, = plan(program, GRAPH, equal_reads(300, 80), l1_prefix=0, has_long=has_long)
        assert has(one, family="flat", has_dead=has_long, wide_d=0, dbg=0, tiles=2), one
        one, = plan(program, GRAPH, equal_reads(300, 80), has_long=has_long)     # (without the hook such a batch takes the prefix form)
        assert has(one, family="prefix", k17=1, c=15), one
    # l1_plain: no pipelined tile loop, no regular tiles
    for facts in (equal_reads(300, 150, packed=1), equal_reads(300, 151), mixed_reads(MIXED), dict(mixed_reads(MIXED), l1_prefix=0),
                  dict(equal_reads(300, 150), n1=573)):
        launches = plan(program, GRAPH, facts, l1_plain=1)
        assert len(launches) == 1 and has(launches[0], k17=0, reg=0, pipe=0, n_reads=300), launches


def test_kfreq_direct_blocks(program):
    kfreq = dict(GRAPH, kfreq=1, kf=2, kmer_size=17)
    one, = plan(program, kfreq, equal_reads(300, 150, packed=1))
    assert has(one, family="uniform", wide_d=3, c=15, ragged=0, reg=0, lin=0, k17=0, n_reads=300), one
    one, = plan(program, kfreq, equal_reads(300, 153, packed=1))      # 137 windows: 9 lanes of 16
    assert has(one, family="uniform", wide_d=3, c=16, ragged=0, reg=0, k17=0), one
    # ragged lengths: the plain 64-bit uniform form -- once the prefix form, which comes first for such a batch, is switched off
    one, = plan(program, kfreq, mixed_reads(MIXED), l1_prefix=0)
    assert has(one, family="uniform", wide_d=2, c=15, ragged=1, k17=0, reg=0), one
    one, = plan(program, kfreq, mixed_reads(MIXED))
    assert has(one, family="prefix", wide_d=2, c=15, k17=0), one


def test_wide_record_engine(program):
    wide = dict(wide=1, wrec=1, kmer_size=63, max_read_len=250, size=144 << 20)
    seen = set()
    for length in (100, 120, 150, 151, 200, 250):
        q = (length - 63 + 1 + 7) // 8
        fits = (1024 // q + 2) * length + 96 <= (W_PIPE_PK_WORDS - 8) * 16
        one, = plan(program, wide, equal_reads(300, length))
        assert has(one, family="wide-uniform", wide_d=0, pipe=int(fits), Q=q, n_lanes=300 * q, tiles=(300 * q + 1023) // 1024), (length, one)
        one, = plan(program, wide, equal_reads(300, length), wide_l1_plain=1)
        assert has(one, family="wide-uniform", pipe=0), (length, one)
        seen.add(fits)
    assert seen == {False, True}
    for has_long in (0, 1):
        one, = plan(program, wide, mixed_reads(MIXED), has_long=has_long)
        assert has(one, family="wide-flat", has_dead=has_long, wide_d=0), one
    for size, wide_d in ((1 << 31, 1), (1 << 32, 2)):
        assert plan(program, wide, equal_reads(300, 150), size=size)[0]["wide_d"] == wide_d
        assert plan(program, wide, mixed_reads(MIXED), size=size)[0]["wide_d"] == wide_d


def list_rows(program):
    res = run(program, ["rows"])
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])   # (1: two equal rows)
    rows = [l for l in res.stdout.splitlines() if l.startswith("row ")]
    counts = {l.split()[1]: int(l.split()[2]) for l in res.stdout.splitlines() if l.startswith("count ")}
    return rows, counts


def test_lists_have_the_rows_of_the_library_and_no_row_twice(program):
    rows, counts = list_rows(program)
    assert counts == ROWS
    assert len(rows) == sum(ROWS.values()) == 110 and len(set(rows)) == len(rows)


# ---- the table of cases that tests/test_l1_forms_gpu.py runs on the GPU (tests/l1_form_cases.py) -------------------------------------

def handle_facts(case):
    """the facts of the handle the case creates, without a device: the level-1 bucket count the planner gives the real table size
    (dbgk_plan_partition), `kf` and the direct-block geometry as dbgk_host_create.h / dbgk_host_partition.h set them"""
    from dbg_assembly_amd import capi
    import l1_form_cases as LC
    if case.engine == "kfreq":       # expected_kmers > 0 and k >= 13: direct blocks, size = 4^k, level-1 bucket = slot >> r
        bits = 2 * case.k
        r = max(20, min(26, bits - 8))
        return dict(part=1, kfreq=1, kf=2, kmer_size=case.k, max_read_len=case.max_read_len, n1=(1 << bits) >> r, geom_size=1 << bits, size=1 << bits)
    size = capi.find_next_prime_ref(LC.SLOTS[case.width])
    if case.engine == "wide":
        return dict(wide=1, wrec=1, kmer_size=case.k, max_read_len=case.max_read_len, size=size)
    info = capi.plan_partition(size, LC.EXPECTED_KMERS)
    assert info.table_slots == size
    return dict(part=1, kmer_size=case.k, max_read_len=case.max_read_len, n1=info.level1_buckets, geom_size=size, size=size)


def batch_facts(case):
    import l1_form_cases as LC
    lens = [len(r) for r in LC.reads(case)]
    assert sorted(lens) == sorted(LC.lengths(case))
    return dict(n_reads=len(lens), n_bases=sum(lens), uniform_len=lens[0] if len(set(lens)) == 1 else 0, len_max=max(lens),
                has_long=int(max(lens) > case.max_read_len), packed=int(case.entry != "push_reads"))


def test_cases_are_the_rows_of_the_lists(program):
    """one case per row: 110 keys, none missing, none extra; every case is filed under its own row"""
    import l1_form_cases as LC
    rows, _ = list_rows(program)
    cases = LC.cases()
    assert sorted(cases) == sorted(r[len("row "):] for r in rows) and len(cases) == 110
    assert all(c.row == row and row in c.launches for row, c in cases.items())
    assert len(LC.UNSELECTABLE) <= 4 and set(LC.UNSELECTABLE) <= set(cases)
    for row, reason in LC.UNSELECTABLE.items():
        assert " and " in reason and any(w in reason for w in ("slots", "buckets", "k <", "k >=")), (row, reason)


def test_every_case_plans_its_row_on_the_real_handle_facts(program):
    """l1_plan on the facts of the handle the library creates for the case and of the recipe's actual reads gives exactly the
    launches the case expects (times the passes); the named row is among them.  Rows in UNSELECTABLE are the only exceptions."""
    import l1_form_cases as LC
    seen = collections.Counter()
    for row, case in sorted(LC.cases().items()):
        if row in LC.UNSELECTABLE:
            continue
        assert case.entry != "push_reads_packed_uniform" or case.recipe[0] == "equal", row
        launches = plan(program, handle_facts(case), batch_facts(case), case.hooks)
        got = ["family=%s wide_d=%d c=%d ragged=%d lin=%d reg=%d packed=%d full=%d k17=%d has_dead=%d pipe=%d dbg=%d" % tuple(
            l[f] for f in "family wide_d c ragged lin reg packed full k17 has_dead pipe dbg".split()) for l in launches]
        assert got * case.passes == case.launches and row in got, (row, case, got)
        if "reg=1" in row:           # two whole regular tiles of 128 reads, then the 44 reads behind them
            assert [(l["first_read"], l["n_reads"], l["Q"]) for l in launches] == [(0, 256, 8), (256, 44, 8)], launches
        seen[(case.engine, case.width)] += 1
    # the tiers: small tables / tables of 2^31 and of 2^32 slots and more
    assert seen == {("graph", 0): 32, ("kfreq", 0): 14, ("wide", 0): 4, ("graph", 1): 32, ("wide", 1): 4, ("graph", 2): 20, ("wide", 2): 4}, seen


def test_case_reads_hold_what_makes_rows_go_wrong():
    """every read set: both strands of a small genome, a read some tens of times, poly-A and poly-T, N, lower case, one other byte;
    mixed lengths: a read whose last lane holds a single window"""
    import l1_form_cases as LC
    for row, case in LC.cases().items():
        reads = LC.reads(case)
        assert reads == LC.reads(case) and len(reads) == LC.N_READS, row
        count = collections.Counter(reads)
        assert 20 <= max(v for r, v in count.items() if set(r) - set(b"AT")) <= 40, row
        assert any(set(r) == set(b"A") for r in reads) and any(set(r) == set(b"T") for r in reads), row
        assert sum(r.count(b"N") for r in reads) == 1 and sum(r.count(b"*") for r in reads) == 1, row
        assert sum(len(bytes(b for b in r if b not in b"ACGTNacgtn")) for r in reads) == 1 and any(r != r.upper() for r in reads), row
        if case.recipe[0] in ("mixed", "trimmed"):
            assert any((len(r) - case.k + 1) % case.recipe[2] == 1 for r in reads), row


def test_built_library_has_one_kernel_per_row(program, tmp_path):
    from test_kernel_resources import LIB, LLVM, kernel_metadata
    if not os.path.exists(LIB):
        pytest.skip("libdbgk.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("the ROCm LLVM tools are not installed")
    names = list(kernel_metadata(tmp_path))
    assert len(names) > 100, "could not read the kernel descriptors of libdbgk.so"
    _, counts = list_rows(program)
    for family, kernel in KERNEL_OF.items():
        built = [n for n in names if re.search(r"\d%sI" % kernel, n)]
        assert len(built) == len(set(built)) == counts[family], (family, len(built), counts[family])
