"""Generate tests/golden/kmerfreq_stat/{clean,raw,corrected}.json from the three k-mer frequency spectra the reference
ships (test/01.clean_correct/<name>_reads.lib.kmer.freq.stat, written by the original kmerfreq).  Each 1.2 MB file is
65542 lines of which a few hundred carry a non-zero species count, so a fixture holds the header values, those rows
(frequency, species) and the SHA-256 and length of the whole file: the writer under test has to rebuild every byte
from the species column alone.  The fixtures are data; this script needs the reference only when it is run.

    python tests/golden/make_kmerfreq_stat_golden.py /path/to/reference/test/01.clean_correct
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def parse(path):
    raw = open(path, "rb").read()
    lines = raw.decode().split("\n")
    assert lines[-1] == "" and lines[5] == "" and lines[6].startswith("#Kmer_Frequency\t")
    head = [ln.split(": ", 1)[1] for ln in lines[:4]]
    space, occupied = lines[4].split(": ", 1)[1].split("  occupied ratio: ")
    rows = []
    for i, ln in enumerate(lines[7:-1]):
        t = ln.split("\t")
        assert len(t) == 7 and int(t[0]) == i + 1
        if int(t[1]):
            assert int(t[4]) == int(t[0]) * int(t[1])
            rows.append([int(t[0]), int(t[1])])
    out = {"source": os.path.basename(path), "k": int(head[0]), "max_freq": int(head[1]), "individuals": int(head[2]),
           "species": int(head[3]), "space": int(space), "occupied_ratio": occupied, "lines": len(lines) - 1,
           "bytes": len(raw), "sha256": hashlib.sha256(raw).hexdigest(), "rows": rows}
    assert out["max_freq"] == len(lines) - 8 and out["species"] == sum(r[1] for r in rows)
    assert out["individuals"] == sum(r[0] * r[1] for r in rows)   # none of the three is cut off at the last row
    return out


def main():
    src = sys.argv[1]
    d = os.path.join(HERE, "kmerfreq_stat")
    os.makedirs(d, exist_ok=True)
    for name in ("clean", "raw", "corrected"):
        g = parse(os.path.join(src, name + "_reads.lib.kmer.freq.stat"))
        with open(os.path.join(d, name + ".json"), "w") as f:
            f.write(json.dumps({k: v for k, v in g.items() if k != "rows"})[:-1] + ', "rows": [\n'
                    + ",\n".join(json.dumps(r) for r in g["rows"]) + "\n]}\n")
        print(name, g["lines"], "lines,", len(g["rows"]), "non-zero rows, highest frequency", g["rows"][-1][0])


if __name__ == "__main__":
    main()
