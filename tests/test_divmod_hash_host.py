"""CPU: hash_code and divmod_magic_small (dbg_assembly_amd/csrc/dbgk_device.h) through their host branches, in a small stand-alone
program (tests/divmod_hash_host_main.cpp) built with the HIP compiler, its host side under ASan + UBSan.  The program runs alone:
nothing is loaded into Python.

  hash_code            against the reference's values in tests/golden/kat.txt and against the arithmetic definition restated here
  divmod_magic_small   against 128-bit division: ten divisors -- both ends of 2^26 .. 2^31 - 1, 600 000 001 and primes between --
                       with the edge values q d - 1, q d, q d + d - 1 (small q, q around 2^32, the largest q, random q), 0,
                       2^64 - 1, and 10^6 random h each
"""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
M64 = (1 << 64) - 1

DIVISORS = [1 << 26, 67108879, 100000007, 268435459, 536870923, 600000001, 1000000007, 1073741827, 2147483629, (1 << 31) - 1]


def hash_code_py(k):
    """kmerSet.h:105-116, on Python integers"""
    k = (k + (~(k << 32) & M64)) & M64
    k ^= k >> 22
    k = (k + (~(k << 13) & M64)) & M64
    k ^= k >> 8
    k = (k + (k << 3)) & M64
    k ^= k >> 15
    k = (k + (~(k << 27) & M64)) & M64
    k ^= k >> 31
    return k


def is_prime(n):
    if n < 2 or n % 2 == 0:
        return n == 2
    f = 3
    while f * f <= n:
        if n % f == 0:
            return False
        f += 2
    return True


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "the HIP compiler is needed (as for the build)"
    exe = str(tmp_path_factory.mktemp("divmod_hash") / "divmod_hash_host_main")
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dbg_assembly_amd", "csrc"),
           os.path.join(ROOT, "tests", "divmod_hash_host_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def run(exe, args, stdin=""):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")   # (the HIP runtime's own start-up allocations are not this program's)
    return subprocess.run([exe] + args, input=stdin, capture_output=True, text=True, env=env)


def test_hash_code_host_branch_equals_kat_and_definition(program):
    kat = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "kat.txt")):
        f = line.rstrip("\n").split("\t")
        if f[0] == "hash_code":
            kat[int(f[1])] = int(f[2])
    assert len(kat) >= 8
    rng = random.Random(20)
    keys = list(kat) + [0, 1, M64, 1 << 63, (1 << 32) - 1, 1 << 32, (1 << 62) - 1] + [rng.getrandbits(64) for _ in range(2000)] \
        + [rng.getrandbits(64) & ~0xFFFFFFFF for _ in range(50)] + [rng.getrandbits(32) for _ in range(50)]
    res = run(program, ["hash"], "".join("%d\n" % k for k in keys))
    assert res.returncode == 0, res.stderr[-2000:]
    got = [int(x) for x in res.stdout.split()]
    assert len(got) == len(keys)
    for k, h in zip(keys, got):
        assert h == hash_code_py(k), k
        if k in kat:
            assert h == kat[k], k


def test_divmod_magic_small_equals_128_bit_division(program):
    assert len(DIVISORS) == 10 and DIVISORS == sorted(DIVISORS) and DIVISORS[0] == 1 << 26 and DIVISORS[-1] == (1 << 31) - 1
    assert all(is_prime(d) for d in DIVISORS if d not in (1 << 26, 600000001))
    res = run(program, ["div"] + [str(d) for d in DIVISORS])
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    rows = [tuple(int(x) for x in l.split()) for l in res.stdout.splitlines() if l and not l.startswith("#")]
    assert [r[0] for r in rows] == DIVISORS
    for d, checked, bad in rows:
        assert checked >= 1000000 + 2 + 3 * 60 and bad == 0, (d, checked, bad)
