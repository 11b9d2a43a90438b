"""Where a substring occurs in the strings of an index, derived from the strings alone (no restatement of the reference's traversal): the
SET of (sid, pos) that `mem -p` / Rb3Gpu.locate may report for a match -- string sid (sequence sid >> 1, its reverse complement if sid & 1,
the order an index built with both strands holds them in), pos the offset of the occurrence in that string.  Which of them are reported
when the cap is below their number, and in which order, is the reference's business; the recorded outputs pin that."""
import numpy as np


def as_bytes(s):
    """a string of nt6 codes as bytes"""
    if isinstance(s, (bytes, bytearray)):
        return bytes(s)
    return bytes(bytearray(np.asarray(s, dtype=np.uint8).tolist()))


def occurrences(strings, pat):
    """{(sid, pos)} of pattern `pat` (nt6 codes) in `strings` (a list of nt6 strings, sid = place in the list)"""
    pat = as_bytes(pat)
    out = set()
    if not pat:
        return out
    for sid, s in enumerate(strings):
        s = as_bytes(s)
        i = s.find(pat)
        while i >= 0:
            out.add((sid, i))
            i = s.find(pat, i + 1)
    return out


def columns(pairs, match_len, names, lengths):
    """the `-p` columns of a match of match_len symbols for pairs [(sid, pos)]: name:strand:position, the position on the forward strand"""
    out = []
    for sid, pos in pairs:
        s = sid >> 1
        out.append("%s:%s:%d" % (names[s], "-" if sid & 1 else "+", lengths[s] - (pos + match_len) if sid & 1 else pos))
    return out


def parse_line(line):
    """(name, st, en, size, [columns]) of one output line of `mem -p`"""
    f = line.rstrip("\n").split("\t")
    cols = f[5:] if len(f) > 4 else []
    if len(f) > 4:
        assert int(f[4]) == len(cols)
    return f[0], int(f[1]), int(f[2]), int(f[3]), cols


def read_len_gz(path):
    import gzip
    names, lengths = [], []
    for l in gzip.open(path, "rt"):
        f = l.split()
        names.append(f[0]), lengths.append(int(f[1]))
    return names, lengths
