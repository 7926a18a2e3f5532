"""Plain Python restatement of the annotation bin/correct_error_reads appends to every header (host/correct_error_reads.cpp:172,
without the final newline), as csrc/dbgk_annot.h composes it on the device.  Pinned to the reference by tests/test_annot_cpu.py:
joined with the input headers and the restated sequences it gives the text of every golden .correct.fa.gz."""
import numpy as np

LITERALS = (b"\tModifiedBaseNum: ", b"\tFinalReadLength: ", b"\tLeftEndTrim: ", b"\tRightEndTrim: ", b"\tIsDeleted: ")
MAX_SUFFIX = sum(len(x) for x in LITERALS) + 4 * 10 + 3   # four 32-bit numbers and a byte: DBGK_CORR_ANNOT_MAX


def suffixes(rec, lens):
    """records (the fields of dbgk_corr_rec) + the lengths of the records in the compact batch -> (suffix bytes uint8, offsets
    uint64[n + 1])"""
    out, off = [], [0]
    for r, length in zip(rec, lens):
        numbers = ((int(r["one_base"]) + int(r["tree"])) & 0xFFFFFFFF, int(length), int(r["left_trim"]), int(r["right_trim"]), int(r["deleted"]))
        s = b"".join(lit + str(v).encode("ascii") for lit, v in zip(LITERALS, numbers))
        out.append(s)
        off.append(off[-1] + len(s))
    return np.frombuffer(b"".join(out), dtype=np.uint8), np.array(off, dtype=np.uint64)


def split(plane, off):
    b = np.asarray(plane, dtype=np.uint8).tobytes()
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def vectors(plane):
    """the plane as the device holds it: whole 16-byte vectors, the pad of the last one 0"""
    b = np.asarray(plane, dtype=np.uint8).tobytes()
    return np.frombuffer(b + bytes(-len(b) % 16), dtype=np.uint8)
