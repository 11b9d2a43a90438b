"""Python models of `overlap`: which strings of an index overlap, end to start, and by how much.  Two things that share nothing:

- brute force on the strings themselves: a dictionary of every prefix of every string, asked for every suffix of every string -- `Brute`;
- the walk of the engine restated over tests/walk_model.Fm, all strings side by side, one numpy step for all of them -- `walk`: from row a follow LF and feed the
  symbols read into one backward search from [0, n).  Pass p reads the symbol c at the row; c == 0 ends the walk (depth p is the whole string: no overlap); else, where
  p >= min_len, the sentinels inside the interval -- occ0(hi) - occ0(lo) of them -- are the strings that start with the last p symbols of a: the group of depth p, kept
  unless a cap is set and the group is larger; then row and interval are extended by c.  With the early exit a walk ends once its interval is one row.  A step is one
  pass, the one that reads the sentinel included.  Sentinel rank e belongs to the string whose own walk ends on the row that holds that sentinel (`who`).

A record is (a, b, len, len_b): the last len symbols of string a are the first len of string b.  The engine's order: a ascending, len descending, sentinel rank ascending.

Also here: the slices of the emit stage (`slices`), the command's bytes (`text`) and the designed set of the tests (`designed`)."""
import numpy as np

from tests.dedup_model import naive_bwt, rows_of  # noqa: F401  (the rows of a set of sequences and their BWT by a naive sort: the tests take them from here)
from tests import util

MIN_LEN, CAP = 20, 9             # what the designed set is designed for: an overlap of exactly MIN_LEN and one of MIN_LEN - 1, a group of exactly CAP and one of CAP + 1


# ---- brute force ----

class Brute:
    """strs: the string of every row (uint8 arrays of nt6 codes 1..5).  triples(min_len): the set of (a, len, b) with min_len <= len < len(a), len <= len(b) and the
    last len symbols of a equal to the first len of b -- and, as a check of its own, how many there are as a list"""

    def __init__(self, strs):
        self.rows = [np.asarray(s, dtype=np.uint8).tobytes() for s in strs]
        self.starts = {}
        for b, s in enumerate(self.rows):
            for l in range(1, len(s) + 1):
                self.starts.setdefault(s[:l], []).append(b)

    def triples(self, min_len):
        out = []
        for a, s in enumerate(self.rows):
            for l in range(max(min_len, 1), len(s)):
                out += [(a, l, b) for b in self.starts.get(s[len(s) - l:], ())]
        got = set(out)
        assert len(got) == len(out)
        return got

    def groups(self, min_len):
        """{(a, len): partners} of the triples"""
        g = {}
        for a, l, _ in self.triples(min_len):
            g[(a, l)] = g.get((a, l), 0) + 1
        return g


# ---- the walk ----

def who_of(fm):
    """(who, lens): who[e] = the string sentinel rank e belongs to; the length of every string"""
    m = int(fm.acc[1])
    end, seqs = fm.retrieve(np.arange(m))
    who = np.full(m, -1, dtype=np.int64)
    e = fm.occ[0, end].astype(np.int64)
    assert np.unique(e).size == m and (fm.b[end] == 0).all()
    who[e] = np.arange(m)
    return who, np.array([s.size for s in seqs], dtype=np.int64)


def walk(fm, min_len, max_hits=0, early=True):
    """dict: rec (k x 4 int64: a, b, len, len_b, in the engine's order), cnt (records per string), last (largest depth with a kept group, -1: none), lens,
    steps_count, steps_emit (last + 1 per string with records), n_early, n_groups, n_capped_groups, n_capped_hits"""
    m, n = int(fm.acc[1]), fm.n
    acc, occ, b = fm.acc, fm.occ, fm.b
    who, lens = who_of(fm)
    k = np.arange(m, dtype=np.int64)
    lo, hi = np.zeros(m, dtype=np.int64), np.full(m, n, dtype=np.int64)
    cnt, last = np.zeros(m, dtype=np.int64), np.full(m, -1, dtype=np.int64)
    ga, gp, ge, gz = [], [], [], []
    steps = n_early = n_cg = n_ch = 0
    live, p = np.arange(m), 0
    while live.size:
        steps += int(live.size)
        c = b[k[live]].astype(np.int64)
        on, c = live[c != 0], c[c != 0]
        if p >= min_len:
            e0, e1 = occ[0, lo[on]].astype(np.int64), occ[0, hi[on]].astype(np.int64)
            z = e1 - e0
            keep = (z > 0) & ((z <= max_hits) if max_hits > 0 else True)
            over = (z > 0) & ~keep
            n_cg, n_ch = n_cg + int(over.sum()), n_ch + int(z[over].sum())
            ga.append(on[keep]), gp.append(np.full(int(keep.sum()), p, dtype=np.int64)), ge.append(e0[keep]), gz.append(z[keep])
            cnt[on[keep]] += z[keep]
            last[on[keep]] = p
        for x in (k, lo, hi):
            x[on] = acc[c] + occ[c, x[on]]
        assert (hi[on] > lo[on]).all()
        p += 1
        if early:
            one = hi[on] - lo[on] == 1
            n_early += int(one.sum())
            on = on[~one]
        live = on
    ga, gp, ge, gz = (np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in (ga, gp, ge, gz))
    o = np.lexsort((-gp, ga))                                # by a, then the longest overlap first
    ga, gp, ge, gz = ga[o], gp[o], ge[o], gz[o]
    tot = int(gz.sum())
    gi = np.repeat(np.arange(gz.size), gz)
    e = ge[gi] + (np.arange(tot) - np.repeat(np.cumsum(gz) - gz, gz))      # inside a group: ascending sentinel rank
    bb = who[e]
    rec = np.stack([ga[gi], bb, gp[gi], lens[bb]], axis=1) if tot else np.zeros((0, 4), dtype=np.int64)
    return dict(rec=rec, cnt=cnt, last=last, lens=lens, steps_count=steps, steps_emit=int((last[cnt > 0] + 1).sum()), n_early=n_early, n_groups=int(gz.size),
                n_capped_groups=n_cg, n_capped_hits=n_ch)


def triples(rec):
    """the records as the set brute force gives, and that no record is there twice"""
    got = {(int(a), int(l), int(b)) for a, b, l, _ in rec}
    assert len(got) == rec.shape[0]
    return got


def slices(cnt, budget):
    """the emit slices: consecutive strings with records whose records sum to at most the budget, a string with more alone -- the records of every slice"""
    out, tot = [], 0
    for c in cnt[cnt > 0]:
        if tot and tot + c > budget:
            out.append(tot)
            tot = 0
        tot += int(c)
    return out + ([tot] if tot else [])


def text(rec, lens, pair=False):
    """the bytes of `overlap [--pair]`"""
    if pair:
        return b"".join(b"%d\t%c\t%d\t%c\t%d\t%d\t%d\n" % (a >> 1, b"+-"[a & 1], b >> 1, b"+-"[b & 1], l, lens[a], lb) for a, b, l, lb in rec.tolist())
    return b"".join(b"%d\t%d\t%d\t%d\t%d\n" % (a, b, l, lens[a], lb) for a, b, l, lb in rec.tolist())


# ---- inputs ----

def designed(seed=11, both=False):
    """the sequences of the designed set, about 20 k symbols on one strand: 100-symbol reads tiled over a contig at every 25th position; an overlap of exactly
    MIN_LEN and one of MIN_LEN - 1; an overlap of len(a) - 1; a partner that IS the overlap; a periodic string (it overlaps itself at every multiple of its period);
    a read whose end is the reverse complement of its own start and one that ends in a reverse-complement palindrome (with both strands: the record that is its own
    mirror image); an N inside an overlap; groups of exactly 8, 9 (= CAP), 10 (= CAP + 1) and 300 partners, with exact copies among them; a string of one
    symbol; and, on one strand, a string of no symbols"""
    rng = np.random.default_rng(seed)
    g = lambda n: util.random_genome(rng, n)    # noqa: E731
    cat = lambda *x: np.concatenate(x).astype(np.uint8)    # noqa: E731
    contig = g(1500)
    out = [contig[i:i + 100].copy() for i in range(0, 1401, 25)]
    x = g(60)
    out += [x, cat(x[-MIN_LEN:], g(40))]                      # exactly MIN_LEN
    x = g(60)
    out += [x, cat(x[-(MIN_LEN - 1):], g(40))]                # MIN_LEN - 1
    x = g(50)
    out += [x, cat(x[1:], g(10))]                             # len(a) - 1
    x = g(70)
    out += [x, x[-30:].copy()]                                # the partner is the overlap
    out.append(np.tile(g(7), 12))                             # periodic
    h = g(25)
    out.append(cat(h, g(20), util.revcomp(h)))                # its end is the reverse complement of its start
    w = g(15)
    out.append(cat(g(40), w, util.revcomp(w)))                # ends in a palindrome: its suffix starts its own reverse complement
    x = g(60)
    x[-10] = 5
    out += [x, cat(x[-25:], g(20))]                           # an N inside the overlap
    for z in (8, CAP, CAP + 1, 300):                          # the lane loop, the cap
        q = g(40 if z == 300 else 35)
        out.append(cat(g(30), q))
        tails = [g(6) for _ in range(z)]
        tails[1] = tails[0].copy()                            # exact copies among the partners
        if z == 300:
            tails[200], tails[299] = tails[0].copy(), tails[150].copy()
        out += [cat(q, t) for t in tails]
    out.append(np.array([3], dtype=np.uint8))
    if not both:
        out.insert(5, np.zeros(0, dtype=np.uint8))
    return out
