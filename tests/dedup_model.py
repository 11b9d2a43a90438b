"""Python models of `dedup`: which strings of an index are copies of another one or lie inside a longer one.  Two things that share nothing:

- brute force on the strings themselves: substring search on bytes, equality by dictionary -- `Brute`;
- the walk of the engine restated over tests/walk_model.Fm, all strings side by side, one numpy step for all of them -- `walk`, `kinds`: from row r follow LF and
  feed the symbols read into two backward searches, `any` from [0, n) and `suf` from [0, m); at the sentinel occ = |any|, cls = occ0(suf.lo), copies = occ0(suf.hi)
  - cls; with the early exit a walk ends as soon as |any| == 1 (occ = copies = 1, cls = -1).  A step is one pass of the loop, the one that reads the sentinel included.

A unit is a row, or with pair sequence u = rows 2u and 2u + 1 of an index of both strands in input order, judged on row 2u.  Kinds: C contained (occ > copies),
D duplicate (copies > 1 and not the smallest unit of its class), K kept.  The keeper of a unit is the smallest unit of its class, itself where copies == 1.

Also here: the designed set of the tests (`designed`), the BWT of a list of strings by a naive sort (`naive_bwt`), and the command's two outputs (`drop_text`,
`table_text`)."""
import numpy as np

from tests import util

K, D, C = ord("K"), ord("D"), ord("C")


# ---- brute force ----

def _bytes(s):
    return np.asarray(s, dtype=np.uint8).tobytes()


class Brute:
    """strs: the string of every row (uint8 arrays of nt6 codes 1..5).  occ[r]: every place row r's string starts at in any row's string (the empty string: every
    position, the ends included); copies[r]: the rows that hold the same string; inside[r]: one of those places lies in a longer string.  One scan of all the
    strings per distinct string"""

    def __init__(self, strs):
        self.rows = rows = [_bytes(s) for s in strs]
        blob = b"\0".join(rows) + b"\0"
        starts = np.concatenate([[0], np.cumsum([len(x) + 1 for x in rows])])
        count, seen = {}, {}
        for s in rows:
            count[s] = count.get(s, 0) + 1
        for s in count:
            if len(s) == 0:
                seen[s] = (len(blob), any(len(x) > 0 for x in rows))
                continue
            n, inside, p = 0, False, blob.find(s)
            while p >= 0:
                n += 1
                if not inside:
                    t = int(np.searchsorted(starts, p, side="right")) - 1
                    inside = len(rows[t]) > len(s)
                p = blob.find(s, p + 1)
            seen[s] = (n, inside)
        self.occ = np.array([seen[s][0] for s in rows], dtype=np.int64)
        self.copies = np.array([count[s] for s in rows], dtype=np.int64)
        self.inside = np.array([seen[s][1] for s in rows], dtype=bool)

    def kinds(self, pair=False, dup_only=False):
        """(kind, keeper) per unit"""
        m = len(self.rows)
        if pair and m % 2:
            raise ValueError("pair needs an even number of rows")
        first = {}
        for r, s in enumerate(self.rows):
            first.setdefault(s, r >> 1 if pair else r)
        nu = m // 2 if pair else m
        kind, keeper = np.zeros(nu, dtype=np.uint8), np.zeros(nu, dtype=np.int64)
        for u in range(nu):
            r = 2 * u if pair else u
            keeper[u] = first[self.rows[r]]
            kind[u] = C if not dup_only and self.inside[r] else D if self.copies[r] > 1 and keeper[u] != u else K
        return kind, keeper


# ---- the walk ----

def walk(fm, early=True):
    """(rec, n_steps, n_early): rec[r] = (occ, copies, cls) of string r, int64"""
    m, n = int(fm.acc[1]), fm.n
    acc, occ, b = fm.acc, fm.occ, fm.b
    k = np.arange(m, dtype=np.int64)
    al, ah = np.zeros(m, dtype=np.int64), np.full(m, n, dtype=np.int64)
    sl, sh = np.zeros(m, dtype=np.int64), np.full(m, m, dtype=np.int64)
    rec = np.zeros((m, 3), dtype=np.int64)
    steps = n_early = 0
    live = np.arange(m)
    while live.size:
        steps += int(live.size)
        c = b[k[live]].astype(np.int64)
        stop = c == 0
        ids = live[stop]
        cls = occ[0, sl[ids]].astype(np.int64)
        rec[ids, 0], rec[ids, 1], rec[ids, 2] = ah[ids] - al[ids], occ[0, sh[ids]] - cls, cls
        own = occ[0, k[ids]]
        assert ((own >= cls) & (own < cls + rec[ids, 1])).all(), "the walk's own row is not in its class"
        on, c = live[~stop], c[~stop]
        for x in (al, ah, sl, sh, k):
            x[on] = acc[c] + occ[c, x[on]]
        assert (ah[on] > al[on]).all() and (sh[on] > sl[on]).all()
        if early:
            uniq = ah[on] - al[on] == 1
            rec[on[uniq]] = (1, 1, -1)
            n_early += int(uniq.sum())
            on = on[~uniq]
        live = on
    return rec, steps, n_early


def kinds(rec, pair=False, dup_only=False):
    """(kind, keeper) per unit from the records of `walk`; ValueError where pair does not fit the index"""
    m = rec.shape[0]
    if pair and m % 2:
        raise ValueError("pair needs an even number of rows")
    unit = np.arange(m) >> 1 if pair else np.arange(m)
    keep = np.full(max(m, 1), m, dtype=np.int64)
    multi = np.flatnonzero(rec[:, 1] > 1)
    np.minimum.at(keep, rec[multi, 2], unit[multi])
    if pair and not np.array_equal(rec[0::2, :2], rec[1::2, :2]):
        raise ValueError("the rows of a unit disagree: not an index of both strands")
    r = rec[0::2] if pair else rec
    nu = r.shape[0]
    u = np.arange(nu)
    keeper = np.where(r[:, 1] > 1, keep[np.maximum(r[:, 2], 0)], u)
    kind = np.full(nu, K, dtype=np.uint8)
    kind[(r[:, 1] > 1) & (keeper != u)] = D
    if not dup_only:
        kind[r[:, 0] > r[:, 1]] = C
    return kind, keeper


def drop_text(kind):
    """the bytes of `dedup`: the units to drop, ascending"""
    return b"".join(b"%d\n" % u for u in np.flatnonzero(np.asarray(kind) != K))


def table_text(kind, keeper, rec, pair=False):
    """the bytes of `dedup --table`: unit, kind, keeper, occ, copies"""
    r = rec[0::2] if pair else rec
    return b"".join(b"%d\t%c\t%d\t%d\t%d\n" % (u, kind[u], keeper[u], r[u, 0], r[u, 1]) for u in range(len(kind)))


# ---- inputs ----

def naive_bwt(strs):
    """the BWT of the strings in input order by sorting all their suffixes: key = (the suffix up to and including its sentinel, the string's number)"""
    keys = []
    for i, s in enumerate(strs):
        t = _bytes(s) + b"\0"
        keys += [(t[p:], i, t[p - 1] if p else 0) for p in range(len(t))]
    keys.sort(key=lambda x: (x[0], x[1]))
    return np.array([x[2] for x in keys], dtype=np.uint8)


def rows_of(seqs, both):
    """the strings of the index's rows: every sequence, with both its reverse complement behind it"""
    out = []
    for s in seqs:
        out.append(np.asarray(s, dtype=np.uint8))
        if both:
            out.append(util.revcomp(out[-1]))
    return out


def designed(seed=7, both=False):
    """the sequences of the designed set, about 10 k symbols: contigs; substrings of them at the start, at the end and inside; substrings of a reverse complement
    only; reads with exact copies; a copy of a reverse complement; two palindromes, one of them twice; strings that differ in their first or their last symbol only;
    a string with an N and a substring across that N; NN; and, on one strand, a string of no symbols (a reverse complement of nothing is nothing: with both strands
    its two rows would be a class of their own, which is the palindromes' case already)"""
    rng = np.random.default_rng(seed)
    g = lambda n: util.random_genome(rng, n)    # noqa: E731
    contigs = [g(int(rng.integers(500, 1100))) for _ in range(9)]
    out = list(contigs)
    for i, c in enumerate(contigs[:6]):                       # substrings: start, end, inside -- and one of them twice
        ln = int(rng.integers(20, 120))
        a = int(rng.integers(1, c.size - ln - 1))
        out += [c[:ln].copy(), c[c.size - ln:].copy(), c[a:a + ln].copy()]
        if i % 3 == 0:
            out.append(c[a:a + ln].copy())
    for c in contigs[6:9]:                                    # of the reverse complement only
        rc = util.revcomp(c)
        out.append(rc[7:7 + int(rng.integers(30, 90))].copy())
    reads = [g(int(rng.integers(40, 150))) for _ in range(8)]
    for i, r in enumerate(reads):                             # exact copies, next to each other and apart
        out.append(r)
        if i < 6:
            out.append(r.copy())
    out += [reads[0].copy(), reads[1].copy(), reads[2].copy(), reads[0].copy()]
    out.append(util.revcomp(reads[6]))                        # a copy of a reverse complement
    h1, h2 = g(31), g(18)
    p1, p2 = np.concatenate([h1, util.revcomp(h1)]), np.concatenate([h2, util.revcomp(h2)])
    out += [p1, p2, p2.copy()]                                # palindromes
    x = g(77)
    xf, xl = x.copy(), x.copy()
    xf[0], xl[-1] = x[0] % 4 + 1, x[-1] % 4 + 1
    out += [x, xf, xl]                                        # first or last symbol only
    wn = g(90)
    wn[40] = 5
    out += [wn, wn[30:55].copy(), np.array([5, 5], dtype=np.uint8)]
    if not both:
        out.insert(11, np.zeros(0, dtype=np.uint8))
    return out
