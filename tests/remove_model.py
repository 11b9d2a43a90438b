"""`remove` restated in numpy: the LF walk of every string taken out marks the rows it stands on -- the row whose symbol is the sentinel
included -- and the BWT of what stays is the old BWT without the marked rows.  The parser of the command's arguments, restated as well.  Test
infrastructure only."""
import re

import numpy as np


class Fm:
    """rank tables of a plain BWT (nt6 codes): occ[c][k] = the number of c in b[:k]"""

    def __init__(self, b):
        self.b = np.ascontiguousarray(b, dtype=np.uint8)
        self.n = int(self.b.size)
        self.cnt = np.bincount(self.b, minlength=6)[:6].astype(np.int64)
        self.acc = np.concatenate([[0], np.cumsum(self.cnt)]).astype(np.int64)
        self.occ = [np.concatenate([[0], np.cumsum(self.b == c)]).astype(np.int64) for c in range(6)]

    def lf(self, k):
        c = int(self.b[k])
        return c, int(self.acc[c] + self.occ[c][k])


def mark(fm, rows):
    """the bitmap of `remove`: True at every row the walks of the strings `rows` (numbers below acc[1]; duplicates collapse) stand on.  Returns (marked,
    steps): steps = the sum of len + 1 over the distinct strings"""
    m = int(fm.acc[1])
    marked = np.zeros(fm.n, dtype=bool)
    steps = 0
    for r in sorted(set(int(x) for x in rows)):
        if not 0 <= r < m:
            raise ValueError("row %d is outside [0, %d)" % (r, m))
        k = r
        while True:
            assert not marked[k], "two walks on one row"
            marked[k] = True
            steps += 1
            c, k2 = fm.lf(k)
            if c == 0:
                break
            k = k2
    return marked, steps


def remove(b, rows):
    """the plain BWT without the strings `rows`, and the deleted symbols per letter"""
    fm = Fm(b)
    marked, steps = mark(fm, rows)
    gone = np.bincount(fm.b[marked], minlength=6)[:6]
    assert int(marked.sum()) == steps and int(gone[0]) == len(set(int(x) for x in rows))     # the check the engine makes before it rebuilds
    if int(gone[0]) >= int(fm.acc[1]):
        raise ValueError("nothing would be left")
    return fm.b[~marked].copy(), gone.astype(np.int64)


def compact_positions(marked, group=8192):
    """the rank/select of the compaction as the engine does it: per group of rows the marked rows in front of it, and for every kept row its new
    position = row - (marked rows in front of its group) - (marked rows in front of it inside the group)"""
    n = marked.size
    ng = -(-n // group)
    per = np.add.reduceat(marked.astype(np.int64), np.arange(0, max(n, 1), group)) if n else np.zeros(0, dtype=np.int64)
    pre = np.concatenate([[0], np.cumsum(per)])[:ng + 1]
    rows = np.flatnonzero(~marked)
    inside = np.cumsum(marked) - marked        # marked rows in front of every row
    pos = rows - inside[rows]
    return pre, rows, pos


_ARG = re.compile(r"^([0-9]+)(?:-([0-9]+))?$")


def parse_rows(arg):
    """an argument of `remove`: `A` or `A-B` (inclusive, A <= B), decimal digits alone -- (A, B), or None: nothing is guessed"""
    m = _ARG.match(arg)
    if not m:
        return None
    def num(s):
        v = 0
        for ch in s:
            if v > (1 << 58):      # (a number that would not fit 63 bits is no row)
                return None
            v = v * 10 + int(ch)
        return v
    a = num(m.group(1))
    b = num(m.group(2)) if m.group(2) is not None else a
    if a is None or b is None or b < a:
        return None
    return a, b


def expand(args, n_strings, pair=False):
    """the rows of a command line: every argument through parse_rows; pair: a number i is sequence i, rows 2i and 2i + 1.  ValueError for an argument
    that is none, a row outside [0, n_strings), or no row at all"""
    rows = []
    for x in args:
        p = parse_rows(x)
        if p is None:
            raise ValueError("'%s' is neither a row number nor a range" % x)
        a, b = p
        if pair:
            a, b = 2 * a, 2 * b + 1
        if b >= n_strings:
            raise ValueError("row %d is outside the index" % b)
        rows += range(a, b + 1)
    if not rows:
        raise ValueError("no row to remove")
    return rows
