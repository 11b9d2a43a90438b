"""The GPU suffix sorter (rb3sort_bwt, rb3gpu_sort.hip) restated round by round in numpy: prefix doubling over a compacted list of
unresolved suffixes, with a census of what k_s_wsort does with every round's list (pure bookkeeping on the group heads).

The truth is brute_sa(): the definition in the header comment of rb3gpu_sort.hip (the i-th sentinel below the (i+1)-th, every sentinel
below A, a suffix read up to and including its sentinel).  `broken` swaps one rule for a wrong copy (tests/test_cpu_sort.py)."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

from tests import util

H0, H0_LONG = 20, 16          # RB3S_H0, RB3S_H0_LONG
CENSUS = ("skipped", "end_in_chunk", "end_in_next", "flag_large", "span_1", "span_2_64", "span_65_126", "span_127", "mixed_rounds", "largest", "to_device_sort")
FAMILY = (2, 63, 64, 65, 127, 128, 129, 200, 1000)
COPIES = (63, 64, 65, 127, 128, 129)
HOMOPOLYMER = (1, 19, 20, 21, 39, 40, 41, 4095, 4096, 4097)
MIX = (3, 129, 70, 64, 5, 300, 127)


def _census(heads, nu, cs):
    """k_s_wsort on a list of nu elements whose groups start at heads[]: wave c takes the groups that start in [64c, 64c + 64)"""
    sizes = np.append(heads[1:], nu) - heads
    cs["largest"] = max(cs["largest"], int(sizes.max()))
    wave = large = 0
    for base in range(0, nu, 64):
        a, b, c = (int(x) for x in np.searchsorted(heads, [base, base + 64, base + 128]))
        if a == b:                                   # Rc == 0: the whole chunk continues a group
            cs["skipped"] += 1
            continue
        if base + 64 > nu:                           # Vc: the list ends inside the chunk
            E, key = nu, "end_in_chunk"
        elif c > b or base + 128 > nu:               # Hn: a head, or the list end, in the next 64 positions
            E, key = (int(heads[b]) if c > b else nu), "end_in_next"
        else:                                        # neither: the last group that starts here is large, only its head is flagged
            E, key = int(heads[b - 1]), "flag_large"
            large += 1
            cs["to_device_sort"] += int(sizes[b - 1])
        cs[key] += 1
        L = E - int(heads[a])
        assert 0 <= L <= 127
        if L > 0:
            wave += 1
            cs["span_1" if L == 1 else "span_2_64" if L <= 64 else "span_65_126" if L <= 126 else "span_127"] += 1
    cs["mixed_rounds"] += int(wave > 0 and large > 0)
    return wave, large


def _heads(change):   # index of the first element of every element's group (the inclusive max-scan of k_s_heads / k_s_heads2)
    return np.maximum.accumulate(np.where(change, np.arange(change.size), 0))


def _unresolved(hidx):   # members of (sub-)groups that still have several elements
    i = np.arange(hidx.size)
    return ~((hidx == i) & np.append(hidx[1:] == i[1:], True))


def sort(text, broken=None):
    text = np.ascontiguousarray(text, dtype=np.uint8)
    n = text.size
    assert n > 0 and text[-1] == 0 and text.max() <= 5
    sid, sentpos = np.cumsum(text == 0) - (text == 0), np.flatnonzero(text == 0)   # sentinels before p; position of the k-th sentinel
    assert n == 1 or (np.diff(np.append(-1, sentpos)) > 1).all()   # empty strings are out of contract (the lone sentinel is pinned on the GPU)
    d_all = sentpos[sid] - np.arange(n)                          # symbols before p's sentinel
    h0 = H0_LONG if n // sentpos.size > 4096 else H0
    pad = np.concatenate([text, np.zeros(h0, dtype=np.uint8)]).astype(np.uint64)
    key = np.zeros(n, dtype=np.uint64)
    for t in range(h0):                                          # round 0: h0 symbols, 3 bits each, cut after the first sentinel
        sym = pad[t:t + n] if broken == "nocut" else np.where(t <= d_all, pad[t:t + n], 0)
        key |= sym.astype(np.uint64) << np.uint64(3 * (h0 - 1 - t))
    sa = np.argsort(key, kind="stable")
    hidx = _heads(np.append(True, key[sa][1:] != key[sa][:-1]))
    rank = np.empty(n, dtype=np.int64)
    rank[sa] = hidx
    lst = sa[_unresolved(hidx)]
    cs, per_round, h, rounds = dict.fromkeys(CENSUS, 0), [], h0, 0
    while lst.size:
        rounds += 1
        assert rounds <= 40                                      # where the driver gives up
        nu, r, i = lst.size, rank[lst], np.arange(lst.size)
        s = 0 if broken == "sid0" else sid[lst]
        near = d_all[lst] <= h if broken == "le" else d_all[lst] < h
        sec = np.where(near, s, rank[np.minimum(lst + h, n - 1)])     # k_s_key2
        gh = _heads(np.append(True, r[1:] != r[:-1]))
        per_round.append(_census(np.flatnonzero(gh == i), nu, cs))
        o = np.lexsort((-i if broken == "reverse" else i, sec, r))   # every group by sec, ties in list order; the groups stay in place
        lst, sec = lst[o], sec[o]
        sh = _heads((gh == i) | np.append(True, sec[1:] != sec[:-1]))
        sa[r + i - gh] = lst                                     # final slot: old rank + index in the group
        rank[lst] = r + (i if broken == "index" else sh) - gh    # new rank: old rank + index of the first with the same sec
        lst = lst[_unresolved(sh)]
        h *= 2
    tw = (rank.astype(np.uint64) << np.uint64(3)) | np.append(np.uint8(0), text[:-1]).astype(np.uint64)
    return SimpleNamespace(text=text, n=n, h0=h0, rounds=rounds, sa=sa.astype(np.uint32), isa=rank, bwt=text[sa - 1], tw=tw, census=cs,
                           per_round=per_round, ckrow=lambda step: rank[::step].copy())


def brute_sa(text):
    """plain sort of the suffixes by the definition: sentinel i becomes the symbol i - n_strings (< 0 < A), and ends its suffix"""
    t, z = [int(x) for x in text], [p for p, x in enumerate(text) if x == 0]
    for i, p in enumerate(z):
        t[p] = i - len(z)
    end = np.searchsorted(z, np.arange(len(t)))                  # z[end[p]]: the first sentinel at or after p
    return np.array(sorted(range(len(t)), key=lambda p: t[p:z[end[p]] + 1]), dtype=np.uint32)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def family(rng, c):
    """c strings = one random 50-symbol prefix + c distinct random 30-symbol tails, shuffled"""
    pre, tails = util.random_genome(rng, 50), {}
    while len(tails) < c:
        t = util.random_genome(rng, 30)
        tails[t.tobytes()] = np.concatenate([pre, t])
    return [list(tails.values())[i] for i in rng.permutation(c)]


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> text (forward strands only, except both_*), read-only"""
    f = {}
    for c in FAMILY:
        f["family_%d" % c] = util.make_text(family(_rng("family_%d" % c), c), True, False)
    for c in COPIES:
        g = util.random_genome(_rng("copies_%d" % c), 90)
        f["copies_%d" % c] = util.make_text([g] * c, True, False)
    rng = _rng("mix")
    f["mix"] = util.make_text([s for c in MIX for s in family(rng, c)], True, False)
    for L in HOMOPOLYMER:
        f["homopolymer_%d" % L] = util.make_text([np.full(L, 1, dtype=np.uint8)], True, False)
    for L in (4095, 4096):
        rng = _rng("len%dx3" % L)
        g = util.random_genome(rng, L)
        f["len%dx3" % L] = util.make_text([g, util.mutate(rng, g, 0.01), g], True, False)    # a string, a 1 % mutant, an exact copy
    f["singles"] = util.make_text([np.array([x], dtype=np.uint8) for x in (1, 2, 3, 4, 5, 1, 1, 5)], True, False)
    f["one_symbol"] = np.array([1, 0], dtype=np.uint8)
    f["both_family_129"] = util.make_text(family(_rng("family_129"), 129), True, True)
    f["both_copies_65"] = util.make_text([util.random_genome(_rng("copies_65"), 90)] * 65, True, True)
    for t in f.values():
        t.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def model(name):
    return sort(fixtures()[name])
