"""The PARSE stage's rule in plain Python (include/dbgk.h, PARSE section), line by line as both host readers apply it
(dbg_assembly_amd/host/reads_io.h, host/clean_common.h: RecordBatch::fill): no maps, no scan -- a header takes the lines behind it.
parse() is one chunk, stream() a text in chunks with the carry-over.  tests/test_parse_cpu.py anchors it to those readers."""
import numpy as np

REC_DTYPE = np.dtype([(f, "<u4") for f in ("head_pos", "head_len", "seq_pos", "seq_len", "qual_pos", "qual_len")])
COUNTERS = ("n_records", "n_lines", "ignored_lines", "consumed", "n_bases", "max_len", "mismatched")
SUMMED = ("n_records", "n_lines", "ignored_lines", "n_bases", "mismatched")   # over the chunks of a stream: those of the whole text


def lines_of(text):
    """-> [(start, length, ends with a newline)]; a '\\r' belongs to its line; bytes behind the last newline are a line"""
    out, pos = [], 0
    while pos < len(text):
        end = text.find(b"\n", pos)
        if end < 0:
            out.append((pos, len(text) - pos, False))
            break
        out.append((pos, end - pos, True))
        pos = end + 1
    return out


def planes(reads):
    """reads back to back in whole 16-byte vectors, the pad 0 -> (plane uint8, offsets uint64[n + 1])"""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64) if reads else []
    total = int(off[-1])
    plane = np.zeros(-(-total // 16) * 16, dtype=np.uint8)
    plane[:total] = np.frombuffer(b"".join(reads), dtype=np.uint8)
    return plane, off


def parse(text, fmt, with_quals=False, last=True):
    """-> dict: records [(head, seq, qual)] as the text has them; bases / quals (None without a plane) / offsets as the batch has
    them; recs (REC_DTYPE); info (COUNTERS)"""
    text = bytes(text)
    assert fmt in (1, 2) and not (with_quals and fmt != 1)
    marker, per = (b"@", 4) if fmt == 1 else (b">", 2)
    lines = [l for l in lines_of(text) if last or l[2]]
    missing = (len(text), 0, False)
    records, recs, ignored, i = [], [], 0, 0
    while i < len(lines):
        start, length, _ = lines[i]
        if length == 0 or text[start:start + 1] != marker:
            ignored += 1
            i += 1
            continue
        if not last and i + per > len(lines):
            break   # the chunk does not hold every line of this record
        head, seq = lines[i], (lines[i + 1] if i + 1 < len(lines) else missing)
        qual = (lines[i + 3] if i + 3 < len(lines) else missing) if fmt == 1 else (0, 0, False)
        recs.append((head[0], head[1], seq[0], seq[1], qual[0], qual[1]))
        records.append(tuple(text[a:a + n] for a, n, _ in (head, seq, qual)))
        i += per
    if last:
        consumed, n_lines = len(text), len(lines)
    elif i < len(lines):
        consumed, n_lines = lines[i][0], i
    else:
        consumed, n_lines = (lines[-1][0] + lines[-1][1] + 1 if lines else 0), len(lines)
    mismatched = sum(1 for _, s, q in records if with_quals and len(s) != len(q))
    keep = [not (with_quals and len(s) != len(q)) for _, s, q in records]
    bases, offsets = planes([s if k else b"" for (_, s, _), k in zip(records, keep)])
    quals = planes([q if k else b"" for (_, _, q), k in zip(records, keep)])[0] if with_quals else None
    lens = np.diff(offsets.astype(np.int64))
    info = dict(n_records=len(records), n_lines=n_lines, ignored_lines=ignored, consumed=consumed, n_bases=int(offsets[-1]),
                max_len=int(lens.max()) if len(lens) else 0, mismatched=mismatched)
    return dict(records=records, bases=bases, quals=quals, offsets=offsets, recs=np.array(recs, dtype=REC_DTYPE).reshape(-1), info=info)


def stream(text, fmt, chunk_bytes, with_quals=False):
    """the text in windows of chunk_bytes, each chunk = what the one before left unconsumed + the next window; the last window is
    the last chunk (capi.Parser.stream does the same on a file) -> [(chunk text, parse() of it)]"""
    text = bytes(text)
    windows = [text[a:a + chunk_bytes] for a in range(0, len(text), chunk_bytes)] or [b""]
    out, carry = [], b""
    for w, window in enumerate(windows):
        chunk = carry + window
        got = parse(chunk, fmt, with_quals, last=w == len(windows) - 1)
        out.append((chunk, got))
        carry = chunk[got["info"]["consumed"]:]
    return out


def joined(parts):
    """the batches of a stream as one -> (records, info summed over SUMMED)"""
    records = [r for _, got in parts for r in got["records"]]
    return records, {f: sum(got["info"][f] for _, got in parts) for f in SUMMED}
