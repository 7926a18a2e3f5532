"""GPU steps of tests/test_stage_lifecycle_gpu.py, each run in a child process of its own under a time limit:
    python tests/stage_lifecycle_gpu_steps.py open_close | bad_device | regrow
Prints one JSON line of findings; exits non-zero on a mismatch."""
import ctypes
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_restatement as DR  # noqa: E402
import format_cases as FC  # noqa: E402
import inflate_cases as IC  # noqa: E402
import parse_cases as PC  # noqa: E402
import parse_restatement as PR  # noqa: E402
from format_gpu_steps import check as check_format  # noqa: E402
from parse_gpu_steps import check as check_parse  # noqa: E402

DESTROYS = ("corr", "map", "clean", "pair", "parse", "fmt", "gz", "inf", "link", "fill", "super", "contig")


def stage_classes(capi):
    """every stage class of capi -> {name: a call that makes one on device 0}"""
    return {"Corrector": lambda: capi.Corrector(k=9), "Mapper": capi.Mapper, "Pairer": capi.Pairer, "Parser": lambda: capi.Parser(PC.FASTQ, True),
            "Formatter": lambda: capi.Formatter(FC.FASTQ), "Deflater": capi.Deflater, "Inflater": capi.Inflater, "Cleaner": capi.Cleaner,
            "Scaffolder": capi.Scaffolder, "GapFiller": capi.GapFiller, "SuperLinker": capi.SuperLinker,
            "ContigBuilder": lambda: capi.ContigBuilder(31), "ContigBuilder_wide": lambda: capi.ContigBuilder(63, wide=True)}


def open_close():
    """every stage class made on device 0 and closed, twice over, the second close a no-op; the handles of all of them open at once
    and closed in the order they were made; every destroy refuses a null handle"""
    from dbg_assembly_amd import capi
    L = capi.lib()
    res = {}
    for name, make in stage_classes(capi).items():
        for _ in range(2):
            s = make()
            assert s._h
            s.close()
            assert not s._h
            s.close()
        with make() as s:
            assert s._h
        assert not s._h
        res[name] = "closed"
    together = [make() for make in stage_classes(capi).values()]
    for s in together:
        s.close()
    res["together"] = len(together)
    for stage in DESTROYS:
        res[stage + "_destroy_null"] = getattr(L, "dbgk_%s_destroy" % stage)(None)
    return res


def bad_device():
    """every create that takes a device index: the index dbgk_device_count() is DBGK_ERR_HIP with "no usable HIP device"; -1 is
    DBGK_ERR_ARG; a stage parameter out of range is DBGK_ERR_ARG whatever the index"""
    from dbg_assembly_amd import capi
    L = capi.lib()
    n_dev = L.dbgk_device_count()
    assert n_dev >= 1
    z3 = (ctypes.c_int32 * 3)(0, 0, 0)
    # name -> (the create's arguments in front of the index with good parameters, with one bad parameter; None: the index is all it takes)
    creates = {
        "dbgk_corr_create": ((ctypes.byref(capi.CorrParams(9, 17, 2, 17, 5000000, 75)),), (ctypes.byref(capi.CorrParams(20, 17, 2, 17, 5000000, 75)),)),
        "dbgk_map_create": ((ctypes.byref(capi.MapParams(31, 5, 250, 0, 0.97)),), (ctypes.byref(capi.MapParams(32, 5, 250, 0, 0.97)),)),
        "dbgk_clean_create": ((), None),
        "dbgk_pair_create": ((), None),
        "dbgk_parse_create": ((1, 1), (3, 0)),
        "dbgk_fmt_create": ((1, 0), (1, 256)),
        "dbgk_link_create": ((ctypes.byref(capi.LinkParams(0, 3, 400)),), (ctypes.byref(capi.LinkParams(2, 3, 400)),)),
        "dbgk_fill_create": ((ctypes.byref(capi.FillParams(3, z3)),), (ctypes.byref(capi.FillParams(-1, z3)),)),
        "dbgk_super_create": ((ctypes.byref(capi.SuperParams(3, z3)),), (ctypes.byref(capi.SuperParams(-1, z3)),)),
        "dbgk_contig_create": ((ctypes.byref(capi.ContigParams(31, 2, 125, 0)),), (ctypes.byref(capi.ContigParams(32, 2, 125, 0)),)),
        "dbgk_wide_contig_create": ((ctypes.byref(capi.ContigParams(63, 2, 125, 0)),), (ctypes.byref(capi.ContigParams(64, 2, 125, 0)),)),
    }
    res = {}
    for name, (good, bad) in creates.items():
        create = getattr(L, name)
        h = ctypes.c_void_p(1)
        res[name] = {"past_the_last": create(*good, n_dev, ctypes.byref(h))}
        res[name]["error"] = L.dbgk_last_error().decode()
        assert not h.value, name
        res[name]["minus_1"] = create(*good, -1, ctypes.byref(h))
        if bad is not None:
            res[name]["bad_parameter"] = create(*bad, 0, ctypes.byref(h))
            res[name]["bad_parameter_past_the_last"] = create(*bad, n_dev, ctypes.byref(h))
        assert not h.value, name
        # and the good parameters on device 0 make a handle
        assert create(*good, 0, ctypes.byref(h)) == capi.OK and h.value, name
        assert getattr(L, name.replace("wide_", "").replace("_create", "_destroy"))(h) == capi.OK
    return res


def fasta_batch(n, read_len=1):
    """n FASTA records with the header '>' and reads of read_len bases -> the case (tests/format_cases.py)"""
    return FC.build(FC.FASTA, [b">"] * n, [b"ACGT"[i % 4:i % 4 + 1] * read_len for i in range(n)])


def fasta_of_bytes(total):
    """a FASTA case of three records whose text has `total` bytes: the middle read takes what the others leave"""
    rest = total - 2 * 4 - 3   # two records '>\nA\n', and '>' and two newlines of the middle one
    return FC.build(FC.FASTA, [b">"] * 3, [b"A", b"ACGT" * (rest // 4) + b"ACGT"[:rest % 4], b"C"])


def regrow_format(capi, g):
    """FORMAT grows the per-record arrays from n + 1 entries (floor 2^14) and the text from its bytes rounded up to 16, + 64
    (floor 2^20)"""
    res = {}
    tiny = fasta_batch(3, 2)
    with capi.Formatter(FC.FASTA) as f:
        steps = [("tiny_first", tiny)]
        steps += [("records_%d" % (n + 1), fasta_batch(n)) for n in ((1 << 14) - 2, (1 << 14) - 1, 1 << 14)]
        steps += [("tiny_after_records", tiny)]
        steps += [("text_%d" % (t + 64), fasta_of_bytes(t)) for t in ((1 << 20) - 64 - 16, (1 << 20) - 64, (1 << 20) - 64 + 1)]
        steps += [("tiny_last", tiny)]
        for name, c in steps:
            info = f.format(c["text"], c["recs"], c["bases"], c["quals"], c["offsets"], c["suffixes"])
            res[name] = check_format(f, g, info, FC.expected(c), name)["out_bytes"]
    return res


def fasta_lines(n_newlines):
    """FASTA records of two lines, '>r\\nA\\n', with n_newlines newlines: an odd count leaves the last read without one"""
    text = b">r\nA\n" * ((n_newlines + 1) // 2)
    return text if n_newlines % 2 == 0 else text[:-1]


def fasta_tiles(n_bytes):
    """FASTA records with reads of about 4000 bases, n_bytes in all"""
    rec = b">r\n" + b"ACGTTGCAAC" * 400 + b"\n"
    text = rec * (n_bytes // len(rec))
    rest = n_bytes - len(text)
    assert rest == 0 or rest > 4
    return text + (b">r\n" + b"G" * (rest - 4) + b"\n" if rest else b"")


def regrow_parse(capi, g):
    """PARSE grows the per-tile arrays from the tiles of 4096 bytes of text (floor 2^10) and the per-line arrays from newlines + 1
    (floor 2^16)"""
    res = {}
    tiny = b">a\nACGT\n>b\nAC\n"
    with capi.Parser(PC.FASTA) as p:
        steps = [("tiny_first", tiny)]
        steps += [("lines_%d" % (n + 1), fasta_lines(n)) for n in ((1 << 16) - 2, (1 << 16) - 1, 1 << 16)]
        steps += [("tiny_after_lines", tiny)]
        steps += [("tiles_%d" % -(-n // PC.T), fasta_tiles(n)) for n in (((1 << 10) - 1) * PC.T, (1 << 10) * PC.T, (1 << 10) * PC.T + 1)]
        steps += [("tiny_last", tiny)]
        for name, text in steps:
            if name.startswith("lines_"):
                assert text.count(b"\n") + 1 == int(name[6:])
            for last in (True, False):
                check_parse(p, g, p.chunk(text, last), PR.parse(text, PC.FASTA, False, last), (name, last))
            res[name] = len(text)
    return res


def regrow_deflate(capi):
    """DEFLATE grows the per-slot arrays from the members of 65280 bytes of text, + 1 with the end marker (floor 64).  Level 0 against
    the restatement byte for byte; level 2, whose token area grows with the slots, inflated by zlib, and a tiny text against the
    restatement"""
    res = {}
    rng = np.random.default_rng(11)
    text = np.frombuffer(b"ACGT\n", dtype=np.uint8)[rng.integers(0, 5, 64 * DR.PIECE + 1)].tobytes()
    tiny = b"@r1\nACGTACGTACGT\n+\nIIIIHHHHGGGG\n"
    with capi.Deflater(0) as z0, capi.Deflater(2) as z2:
        steps = [("tiny_first", tiny)]
        steps += [("slots_%d" % (m + 1), text[:m * DR.PIECE - 7]) for m in (62, 63, 64)]
        steps += [("slots_66", text), ("tiny_last", tiny)]
        for name, data in steps:
            want, info = DR.deflate(data, 0)
            got = z0.deflate(data)
            assert got == want, (name, IC_first_difference(got, want))
            assert {k: z0.info[k] for k in DR.COUNTERS} == info, (name, z0.info)
            got2 = z2.deflate(data)
            assert gzip.decompress(got2) == data, name
            assert z2.info["n_members"] == info["n_members"] and len(DR.walk(got2)) == info["n_members"] + 1, name
            if len(data) < 100:
                assert got2 == DR.deflate(data, 2)[0], name
            res[name] = info["n_members"] + 1
    return res


def IC_first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], dtype=np.uint8) != np.frombuffer(b[:n], dtype=np.uint8))
    return (len(a), len(b), int(d[0]) if d.size else n)


def regrow_inflate(capi):
    """INFLATE grows the per-member arrays from the members of a call (floor 1024); zlib says what they inflate to"""
    res = {}
    texts = [b"r%d:" % i + b"ACGT"[i % 4:] * (1 + i % 5) for i in range(1025)]
    members = [IC.zmember(t) for t in texts]
    with capi.Inflater() as z:
        for name, n in (("tiny_first", 2), ("members_1023", 1023), ("members_1024", 1024), ("members_1025", 1025), ("tiny_last", 3)):
            data, want = b"".join(members[:n]), b"".join(texts[:n])
            assert gzip.decompress(data) == want
            got, info = z.inflate(data)
            assert got == want, (name, IC_first_difference(got, want))
            assert (info["n_members"], info["consumed"], info["out_bytes"], info["n_bad"]) == (n, len(data), len(want), 0), (name, info)
            assert not z.member_status().any()
            res[name] = n
    return res


def regrow():
    """one handle each of Formatter, Parser, Deflater and Inflater fed batches one below, at and one above each floor of a capacity,
    a tiny batch before, between and after: every output is the restatement's, byte for byte"""
    from dbg_assembly_amd import capi
    with capi.Graph(k=31, table_slots=1009, engine=capi.ENGINE_DIRECT) as g:
        return {"format": regrow_format(capi, g), "parse": regrow_parse(capi, g), "deflate": regrow_deflate(capi), "inflate": regrow_inflate(capi)}


if __name__ == "__main__":
    print(json.dumps({"open_close": open_close, "bad_device": bad_device, "regrow": regrow}[sys.argv[1]]()))
