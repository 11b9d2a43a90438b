"""Python models of `overlap --reduce`: which records of `overlap` no two longer ones imply.  Two things that share nothing:

- the rule on the records (`reduce_records`): with R the records of `overlap`, (a, b, o) is reducible iff some (a, c, o_c) of R has o_c > o and len(c) > o_c, and
  (c, b, len(c) - o_c + o) is in R;
- brute force on the strings themselves (`reduce_strings`): (a, b, o) is reducible iff some c and some o_c with o < o_c < len(a) and o_c < len(c) have
  a[len(a) - o_c:] == c[:o_c] and e = c[o_c:] a prefix of b[o:].  It knows no cap: it is the rule for the uncapped set.

Both take switches that turn the rule into one of its near misses, so that the tests can show that the designed set tells them apart: `overhang=False` drops
len(c) > o_c (a witness that is only a suffix of a), and `strict=False` (strings only) lets o_c == o.  On the records the second near miss changes nothing, and that
is asserted too: with o_c == o the third record would overlap the whole of c, which no record does.

Also here: the designed set of the tests (`designed_reduce`, `designed_cases`) and the random read set (`read_set`)."""
import numpy as np

from tests import util
from tests.overlap_model import CAP, MIN_LEN


# ---- the rule on the records ----

def reduce_records(rec, lens, overhang=True):
    """rec: k x 4 (a, b, len, len_b) in the engine's order (a ascending, len descending); lens: the length of every string.  The keep mask of the records"""
    rec = np.asarray(rec, dtype=np.int64).reshape(-1, 4)
    lens = np.asarray(lens, dtype=np.int64)
    k = rec.shape[0]
    keep = np.ones(k, dtype=bool)
    if k == 0:
        return keep
    a, b, o = rec[:, 0], rec[:, 1], rec[:, 2]
    assert (np.diff(a) >= 0).all() and (np.diff(o)[np.diff(a) == 0] <= 0).all()
    m, w = int(lens.size), int(lens.max()) + 2
    have = np.sort((a * m + b) * w + o)                                           # R as sorted keys
    assert (np.diff(have) > 0).all()
    idx = np.arange(k)
    new_a = np.concatenate([[True], a[1:] != a[:-1]])
    new_g = new_a | np.concatenate([[True], o[1:] != o[:-1]])
    first = np.maximum.accumulate(np.where(new_a, idx, 0))                       # the first record of the same a
    group = np.maximum.accumulate(np.where(new_g, idx, 0))                       # the first record of the same (a, len): the records in front overlap a by more
    n_cand = group - first
    end = np.cumsum(n_cand)
    j0 = 0
    while j0 < k:                                                                # pieces of at most 4 M pairs (a record with more: alone)
        j1 = max(j0 + 1, int(np.searchsorted(end, (end[j0 - 1] if j0 else 0) + (1 << 22), side="right")))
        n = n_cand[j0:j1]
        tot = int(n.sum())
        if tot:
            jj = np.repeat(np.arange(j0, j1), n)
            ii = first[jj] + (np.arange(tot) - np.repeat(np.cumsum(n) - n, n))
            c, oc = b[ii], o[ii]
            want = (c * m + b[jj]) * w + lens[c] - oc + o[jj]
            pos = np.minimum(np.searchsorted(have, want), k - 1)
            hit = have[pos] == want
            if overhang:
                hit &= lens[c] > oc
            keep[jj[hit]] = False
        j0 = j1
    return keep


# ---- brute force on the strings ----

def reduce_strings(strs, min_len, overhang=True, strict=True):
    """(kept, every): the sets of triples (a, len, b) that are kept and that there are, from the strings alone"""
    rows = [np.asarray(s, dtype=np.uint8).tobytes() for s in strs]
    starts = {}
    for i, s in enumerate(rows):
        for n in range(1, len(s) + 1):
            starts.setdefault(s[:n], []).append(i)
    kept, every = set(), set()
    for a, s in enumerate(rows):
        la = len(s)
        ends = [(oc, rows[c][oc:]) for oc in range(1, la) for c in starts.get(s[la - oc:], ()) if len(rows[c]) > oc or not overhang]   # what every c adds behind a
        for o in range(max(min_len, 1), la):
            wit = [e for oc, e in ends if (oc > o if strict else oc >= o)]
            for b in starts.get(s[la - o:], ()):
                every.add((a, o, b))
                tail = rows[b][o:]
                if not any(tail.startswith(e) for e in wit):
                    kept.add((a, o, b))
    return kept, every


# ---- inputs ----

def read_set(seed=5, n_reads=160, read_len=60, genome=1200):
    """random error-free reads of a random genome"""
    rng = np.random.default_rng(seed)
    return util.reads_from(rng, util.random_genome(rng, genome), n_reads, read_len)


def _designed(seed):
    rng = np.random.default_rng(seed)
    g = lambda n: util.random_genome(rng, n)    # noqa: E731
    cat = lambda *x: np.concatenate(x).astype(np.uint8)    # noqa: E731
    other = lambda x: np.uint8(x % 4 + 1)    # noqa: E731
    seqs, cases = [], {}

    def put(*xs):
        i = len(seqs)
        seqs.extend(np.asarray(x, dtype=np.uint8) for x in xs)
        return list(range(i, i + len(xs)))

    def case(name, a, c, b, o, kept, **more):
        cases[name] = dict(a=a, c=c, b=b, o=o, kept=kept, strand=0, **more)

    L = MIN_LEN
    # every case lies on a contig G of its own: a = G[0:60], and with c = G[pc:..], b = G[pb:..] the overlaps are o_c = 60 - pc, o = 60 - pb
    G = g(140)
    a, c, b = put(G[0:60], G[20:80], G[35:95])
    case("chain", a, c, b, 25, False, list=(1, 0))                                # c's list: the one record, the target
    G = g(140)
    a, c, b = put(G[0:60], G[34:89], G[35:95])
    case("next_depth", a, c, b, 25, False)                                        # o_c == o + 1
    G = g(140)
    a, c, b = put(G[0:60], G[20:80], G[60 - L:100])
    case("at_min", a, c, b, L, False)                                             # o == min_len, with a witness
    G = g(140)
    a, c, b = put(G[0:60], G[61 - L:101], G[60 - L:100])
    case("below_min", a, c, b, L, True)                                           # the only other string overlaps a by min_len - 1: no record, no witness
    G = g(140)
    a, c, b = put(G[0:60], G[20:60], G[35:95])
    case("suffix_only", a, c, b, 25, True)                                        # len(c) == o_c: contained in a
    G = g(140)
    a, c, b = put(G[0:60], G[20:80], G[35:80])
    case("ends_with_c", a, c, b, 25, False)                                       # o' == len(b)
    G = g(140)
    a, c, b = put(G[0:60], G[20:80], G[35:75])
    case("beyond_b", a, c, b, 25, True)                                           # e is longer than b[o:]
    G = g(140)
    a, c, b = put(G[0:60], cat(G[20:79], [other(G[79])]), G[35:95])
    case("last_symbol", a, c, b, 25, True)                                        # e differs from b[o:] in its last symbol only
    G = g(140)
    a, c, c2, b = put(G[0:60], G[20:80], G[20:80], G[35:95])
    case("witness_copies", a, c, b, 25, False, c2=c2)
    G = g(140)
    a, c, b, b2 = put(G[0:60], G[20:80], G[35:95], G[35:95])
    case("partner_copies", a, c, b, 25, False)
    case("partner_copies_2", a, c, b2, 25, False)
    s, = put(np.tile(g(7), 12))
    case("periodic_deepest", s, s, s, 77, True)
    case("periodic", s, s, s, 70, False)                                          # its own witness: c == a == b
    # the cap: a group of CAP + 1 partners is left out by -c CAP
    G = g(140)
    a, c, b = put(G[0:60], G[20:80], G[35:95])
    put(*[cat(G[20:60], g(15)) for _ in range(CAP)])                             # with c the CAP + 1 partners of (a, 40)
    case("cap_first", a, c, b, 25, False, capped="kept")
    G = g(140)
    a, c, b = put(G[0:60], G[20:80], G[35:95])
    put(*[cat(G[35:80], g(15)) for _ in range(CAP)])                             # with b the CAP + 1 partners of (c, 45) -- and so of (a, 25): see designed_reduce
    case("cap_third", a, c, b, 25, False, capped="absent")
    # 300 partners at one depth under one deeper witness
    G, E = g(60), g(3)
    tails = [g(10) for _ in range(300)]
    for i, t in enumerate(tails):
        if i % 3 == 0:
            t[:3] = E
        elif np.array_equal(t[:3], E):
            t[2] = other(t[2])
    a, c = put(G, cat(G[32:60], E))
    bs = put(*[cat(G[35:60], t) for t in tails])
    cases["big"] = dict(a=a, c=c, b=bs, o=25, kept=[i % 3 != 0 for i in range(300)], strand=0)
    # the ends of the binary search: c's list of one and of two records, the target first, last and not there
    G = g(140)
    a, c, b, d = put(G[0:60], G[20:100], G[35:75], cat(G[75:100], g(20)))
    case("list1_absent", a, c, b, 25, True, list=(1, None))
    G = g(140)
    a, c, b, d = put(G[0:60], G[20:80], G[35:95], cat(G[58:80], g(20)))
    case("list2_first", a, c, b, 25, False, list=(2, 0))
    G = g(140)
    a, c, b, d = put(G[0:60], G[20:80], G[35:95], cat(G[30:80], g(20)))
    case("list2_last", a, c, b, 25, False, list=(2, 1))
    case("list2_last_d", a, c, d, 30, False, list=(2, 0))
    G = g(140)
    a, c, b, d, d2 = put(G[0:60], G[20:80], cat(G[35:79], [other(G[79])], g(15)), cat(G[30:80], g(20)), cat(G[58:80], g(20)))
    case("list2_absent_mid", a, c, b, 25, True, list=(2, None))                   # 50 and 22 are there, 45 is asked for
    G = g(140)
    a, c, b, d, d2 = put(G[0:60], G[20:80], cat(G[35:79], [other(G[79])], g(15)), cat(G[30:80], g(20)), cat(G[32:80], g(20)))
    case("list2_absent_low", a, c, b, 25, True, list=(2, None))                   # 50 and 48 are there
    G = g(140)
    a, c, b, d = put(G[0:60], G[20:80], cat(G[35:79], [other(G[79])], g(15)), cat(G[35:80], g(20)))
    case("list1_other_rank", a, c, b, 25, True, list=(1, None))                   # (c, d, 45) is there: the same length, another string
    case("list1_other_rank_d", a, c, d, 25, False, list=(1, 0))
    # across the strands: the partner is indexed as its reverse complement
    G = g(140)
    a, c, b = put(G[0:60], G[20:80], util.revcomp(G[35:95]))
    case("strands", a, c, b, 25, False)
    cases["strands"].update(strand=1)                                             # b is row 2 * b + 1; on one strand there is no such record
    return seqs, cases


def designed_reduce(seed=23, both=False):
    """the sequences of the designed set, about 25 k symbols on one strand: every border of the rule as a triple a, c, b of its own on a random contig of its own
    (`designed_cases` says which is which), overlaps around MIN_LEN.  No string of no symbols: sequence i is row i on one strand and rows 2i, 2i + 1 on both, and the
    set is the same for both -- `both` is taken so that the call reads like overlap_model.designed.

    One case cannot be built as first written down: a witness whose THIRD record (c, b, o') lies in a group of CAP + 1 partners while (a, b, o) stays in the capped
    set.  Every string that starts with the last o' symbols of c starts with the last o symbols of a, so the group of (a, o) has at least as many partners and is left
    out with it: with -c CAP the record is not there at all (`capped="absent"`), without a cap it is reducible.  Where the FIRST record (a, c, o_c) is in the group that
    is left out, the record is kept with -c CAP and reducible without (`capped="kept"`)"""
    del both
    return _designed(seed)[0]


def designed_cases(seed=23):
    """{name: a, c, b (sequence numbers; `big`: b is a list), o, kept (without a cap, at MIN_LEN or below), strand (of b on both strands; 1: no record on one strand),
    and where given capped ("kept" / "absent": with -c CAP) and list (the records of c's list at MIN_LEN, the target's place in it or None)}"""
    return _designed(seed)[1]


def row(i, both, strand=0):
    return 2 * i + strand if both else i
