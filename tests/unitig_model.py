"""Python models of `unitig`: the unambiguous paths of the string graph that `overlap --reduce` leaves, spelled.  Three things that share nothing:

- the rule followed one vertex at a time (`sequential`): degrees from the kept records, the simple records as `next`, every chain walked from its head;
- the engine's scheme restated in numpy (`jumping`): pointer jumping along `prev` with (pointer, members in front, symbols in front, smallest row, head), the cycles
  cut in front of their smallest row and ranked once more;
- brute force on the strings alone (`brute_check`): every member lies at its offset in the spelled unitig, the written pieces tile it, and no unitig could have been
  extended at either end by a kept record (those of reduce_model.reduce_strings) without breaking the degree rule.

`sequential` takes switches that turn the rule into one of its near misses (`per_partner`, `self_loops`, `cut_largest`, `strict_mirror`), so that the tests can show
that the designed set tells them apart.

An answer is a dict: `utg` (k x 5: head, tail, members, circ, length, by ascending head), `mem` (n x 3: row, o_in, off, unitig by unitig, by rank), `links`
(j x 5: from unitig, from orientation, to unitig, to orientation, overlap; orientation 1 is `-`), `n_asym` and the counters.  With `pair` and n_asym > 0 the answer
is `refused` and holds the counters of the graph only.

Also here: the designed sets of the tests (`designed`, `SETS`) and the command's bytes (`text`, `gfa`, `table`)."""
import numpy as np

from tests import util
from tests import reduce_model as rm
from tests.overlap_model import MIN_LEN

NONE = -1


# ---- the graph: shared by nothing but the two rules below, each of which builds its own ----

def _degrees(K, m, per_partner=False):
    a, b = K[:, 0], K[:, 1]
    if per_partner:                                                              # the near miss: (a, b, o1) and (a, b, o2) count once
        ab = np.unique(K[:, :2], axis=0) if K.shape[0] else K[:, :2]
        return np.bincount(ab[:, 0], minlength=m), np.bincount(ab[:, 1], minlength=m)
    return np.bincount(a, minlength=m), np.bincount(b, minlength=m)


def _simple_mask(K, m, per_partner=False, self_loops=False):
    dout, din = _degrees(K, m, per_partner)
    s = (dout[K[:, 0]] == 1) & (din[K[:, 1]] == 1)
    if not self_loops:
        s &= K[:, 0] != K[:, 1]
    return s


def _finish(K, lens, pair, simple, chains, n_asym, extra=None, strict_mirror=False):
    """chains: list of (members in order, circ) of EVERY chain; the output filter, the numbering, the layout and the links"""
    m = lens.size
    out = dict(n_strings=m, n_kept=int(K.shape[0]), n_simple=int(simple.sum()), n_asym=int(n_asym), refused=bool(pair and n_asym > 0))
    out.update(extra or {})
    if out["refused"]:
        return out
    assert sorted(v for c, _ in chains for v in c) == list(range(m))               # every vertex belongs to exactly one chain
    o_in = np.zeros(m, dtype=np.int64)
    o_in[K[simple, 1]] = K[simple, 2]
    keep = []
    for c, circ in chains:
        h, t = c[0], c[-1]
        if not pair:
            ok = True
        elif circ:
            ok = h % 2 == 0
        else:
            ok = h < (t ^ 1) if strict_mirror else h <= (t ^ 1)
        if ok:
            keep.append((c, circ))
    keep.sort(key=lambda x: x[0][0])
    uid = np.full(m, NONE, dtype=np.int64)
    utg, mem = [], []
    for u, (c, circ) in enumerate(keep):
        off = 0
        for r, v in enumerate(c):
            o = 0 if r == 0 else int(o_in[v])
            if r:
                off += int(lens[c[r - 1]]) - o
            mem.append((v, o, off))
            uid[v] = u
        utg.append((c[0], c[-1], len(c), circ, off + int(lens[c[-1]])))
    links = []
    for a, b, o in K[~simple, :3].tolist():
        if pair and not a <= (b ^ 1):
            continue
        ends = []
        for v in (a, b):
            if uid[v] >= 0:
                ends += [int(uid[v]), 0]
            else:
                assert pair and uid[v ^ 1] >= 0, "an end on a chain that is not output, whose mirror chain is not output either"
                ends += [int(uid[v ^ 1]), 1]
        links.append(ends + [o])
    out["utg"] = np.array(utg, dtype=np.int64).reshape(-1, 5)
    out["mem"] = np.array(mem, dtype=np.int64).reshape(-1, 3)
    out["links"] = np.array(links, dtype=np.int64).reshape(-1, 5)
    out.update(n_unitigs=len(utg), n_members=len(mem), n_symbols=int(out["utg"][:, 4].sum()), n_cycles=int((out["utg"][:, 3] > 0).sum()),
               n_links=len(links), max_members=int(out["utg"][:, 2].max()) if utg else 0)
    return out


# ---- 1. the rule, one vertex at a time ----

def sequential(K, lens, pair=False, per_partner=False, self_loops=False, cut_largest=False, strict_mirror=False):
    K = np.asarray(K, dtype=np.int64).reshape(-1, 4)[:, :3]
    lens = np.asarray(lens, dtype=np.int64)
    m = lens.size
    simple = _simple_mask(K, m, per_partner, self_loops)
    nxt, prv, o_in = {}, {}, {}
    for a, b, o in K[simple].tolist():
        assert per_partner or (a not in nxt and b not in prv)                     # (the near miss calls two records of one pair simple: the later one stays)
        nxt[a], prv[b], o_in[b] = b, a, o
    n_asym = sum(1 for v, w in nxt.items() if nxt.get(w ^ 1, NONE) != (v ^ 1)) if pair else 0
    chains, seen = [], set()
    for h in range(m):                                                           # the paths, from their heads
        if h not in prv:
            c = [h]
            while c[-1] in nxt:
                c.append(nxt[c[-1]])
            chains.append((c, 0))
            seen.update(c)
    for v in range(m):                                                           # what is left lies on cycles
        if v not in seen:
            c = [v]
            while nxt[c[-1]] != v:
                c.append(nxt[c[-1]])
            seen.update(c)
            i = c.index(max(c) if cut_largest else min(c))
            c = c[i:] + c[:i]
            chains.append((c, o_in[c[0]]))
    return _finish(K, lens, pair, simple, chains, n_asym, strict_mirror=strict_mirror)


# ---- 2. the engine's scheme in numpy ----

def jumping(K, lens, pair=False):
    """the rounds of the engine: every vertex carries (ptr, cnt, sym, mn, root); a round is ptr <- ptr[ptr] with the sums, the minimum and the head taken along.
    Phase 1 ends when nothing is live, or when the live count has stopped falling and 2^rounds >= live (every live vertex then lies on a cycle and has seen all of
    it); the cycles are cut in front of their smallest row and their vertices ranked again.  Also returns n_rounds"""
    K = np.asarray(K, dtype=np.int64).reshape(-1, 4)[:, :3]
    lens = np.asarray(lens, dtype=np.int64)
    m = lens.size
    dout, din = np.bincount(K[:, 0], minlength=m), np.bincount(K[:, 1], minlength=m)
    simple = (dout[K[:, 0]] == 1) & (din[K[:, 1]] == 1) & (K[:, 0] != K[:, 1])
    nxt, prv, o_in, circ = (np.full(m, NONE, dtype=np.int64) for _ in range(4))
    o_in[:], circ[:] = 0, 0
    nxt[K[simple, 0]], prv[K[simple, 1]], o_in[K[simple, 1]] = K[simple, 1], K[simple, 0], K[simple, 2]
    n_asym = 0
    if pair:
        v = np.flatnonzero(nxt >= 0)
        n_asym = int((nxt[nxt[v] ^ 1] != (v ^ 1)).sum())
    idx = np.arange(m)

    def init(who):
        ptr[who] = prv[who]
        has = who[prv[who] >= 0]
        cnt[who], sym[who], mn[who] = 0, 0, who
        cnt[has], sym[has] = 1, lens[prv[has]] - o_in[has]
        root[who] = np.where(prv[who] >= 0, NONE, who)

    def jump():
        v = np.flatnonzero(ptr >= 0)
        q = ptr[v]
        c2, s2, m2, p2 = cnt[v] + cnt[q], sym[v] + sym[q], np.minimum(mn[v], mn[q]), ptr[q]
        r2 = np.where(p2 < 0, root[q], root[v])
        cnt[v], sym[v], mn[v], ptr[v], root[v] = c2, s2, m2, p2, r2
        return int((ptr >= 0).sum())

    ptr, cnt, sym, mn, root = (np.zeros(m, dtype=np.int64) for _ in range(5))
    init(idx)
    rounds, live = 0, int((ptr >= 0).sum())
    while live:
        before, live = live, jump()
        rounds += 1
        if live == before and (1 << rounds) >= live:
            break
    cyc = np.flatnonzero(ptr >= 0)
    if cyc.size:
        heads = cyc[mn[cyc] == cyc]
        circ[heads], o_in[heads] = o_in[heads], 0
        nxt[prv[heads]], prv[heads] = NONE, NONE
        init(cyc)
        live = int((ptr >= 0).sum())
        while live:
            live = jump()
            rounds += 1
    tails = np.flatnonzero(nxt < 0)
    assert int((cnt[tails] + 1).sum()) == m and (root[tails] >= 0).all() and np.unique(root[tails]).size == tails.size
    chains = []
    for t in tails.tolist():
        c = np.flatnonzero(root == root[t])
        c = c[np.argsort(cnt[c])]
        assert np.array_equal(cnt[c], np.arange(c.size)) and c[0] == root[t] and c[-1] == t
        chains.append((c.tolist(), int(circ[c[0]])))
    out = _finish(K, lens, pair, simple, chains, n_asym, extra=dict(n_rounds=rounds))
    if not out["refused"]:                                                       # the layout by the sums of the rounds is the layout by the rule
        assert np.array_equal(out["mem"][:, 2], sym[out["mem"][:, 0]]) and np.array_equal(out["mem"][:, 1], o_in[out["mem"][:, 0]])
    return out


# ---- 3. from the strings alone ----

def spell(ans, strs):
    """the unitigs' symbols, each member's piece [o_in, len) written at off + o_in -- and the pieces tile the unitig exactly"""
    out, at = [], 0
    for h, t, n, circ, ln in ans["utg"].tolist():
        s = np.zeros(ln, dtype=np.uint8)
        end = 0
        for v, o, off in ans["mem"][at:at + n].tolist():
            assert off + o == end, "the pieces do not tile the unitig"
            s[off + o:off + strs[v].size] = strs[v][o:]
            end = off + strs[v].size
        assert end == ln
        out.append(s)
        at += n
    assert at == ans["mem"].shape[0]
    return out


def brute_check(ans, strs, min_len, pair):
    """what has to hold for the strings themselves, with the kept records found by reduce_model.reduce_strings (no cap)"""
    seqs = spell(ans, strs)
    kept, _ = rm.reduce_strings(strs, min_len)
    out_of, into = {}, {}
    for a, o, b in kept:
        out_of.setdefault(a, []).append((b, o))
        into.setdefault(b, []).append((a, o))
    at = 0
    starts, ends = [], []
    for u, (h, t, n, circ, ln) in enumerate(ans["utg"].tolist()):
        mem = ans["mem"][at:at + n].tolist()
        at += n
        assert mem[0][0] == h and mem[-1][0] == t and mem[0][1] == 0 and mem[0][2] == 0
        starts += [x[2] for x in mem]
        ends += [x[2] + strs[x[0]].size for x in mem]
        for (v, o, off), nx in zip(mem, mem[1:] + [None]):
            assert np.array_equal(seqs[u][off:off + strs[v].size], strs[v])      # every member lies at its offset
            if nx is not None:                                                   # inside: the one record out of v, the one record into its successor
                assert out_of[v] == [(nx[0], nx[1])] and into[nx[0]] == [(v, nx[1])] and nx[0] != v
                assert nx[2] > off and nx[2] + strs[nx[0]].size >= off + strs[v].size   # starts strictly increase, ends never decrease
        # the ends: a record that would extend the unitig breaks the degree rule -- or closes the circle
        ext = [(b, o) for b, o in out_of.get(t, []) if len(out_of[t]) == 1 and len(into[b]) == 1 and b != t]
        assert ext == ([(h, circ)] if circ else []), (u, ext)
        ext = [(a, o) for a, o in into.get(h, []) if len(into[h]) == 1 and len(out_of[a]) == 1 and a != h]
        assert ext == ([(t, circ)] if circ else []), (u, ext)
        if circ:
            assert seqs[u][ln - circ:].tobytes() == seqs[u][:circ].tobytes() and h == min(x[0] for x in mem)
    rows = sorted(x for x in ans["mem"][:, 0].tolist())
    if pair:                                                                     # every sequence on exactly one unitig -- or, a self-mirror chain, with both strands on it
        assert len(set(rows)) == len(rows) and {r >> 1 for r in rows} == set(range(len(strs) // 2))
        for u, (h, t, n, circ, ln) in enumerate(ans["utg"].tolist()):
            if not circ and h == (t ^ 1):                                        # its own mirror image: it reads the same on both strands
                assert np.array_equal(seqs[u], util.revcomp(seqs[u]))
    else:
        assert rows == list(range(len(strs)))
    # the links: the kept records that are not inside a chain and do not close a circle
    inside = set()
    at = 0
    for h, t, n, circ, ln in ans["utg"].tolist():
        mem = ans["mem"][at:at + n].tolist()
        at += n
        inside |= {(a[0], b[1], b[0]) for a, b in zip(mem, mem[1:])}
        if circ:
            inside.add((t, circ, h))
    if not pair:
        assert ans["links"].shape[0] == len(kept) - len(inside)
    return seqs


# ---- the command's bytes ----

LETTERS = np.frombuffer(b"$ACGTN", dtype=np.uint8)


def _tags(u):
    return b"\tLN:i:%d\tRC:i:%d" % (u[4], u[2])


def text(ans, seqs):
    return b"".join(b">utg%d" % i + _tags(u) + (b"\tCL:i:%d" % u[3] if u[3] else b"") + b"\n" + LETTERS[s].tobytes() + b"\n"
                    for i, (u, s) in enumerate(zip(ans["utg"].tolist(), seqs)))


def gfa(ans, seqs):
    out = [b"H\tVN:Z:1.0\n"]
    out += [b"S\tutg%d\t" % i + LETTERS[s].tobytes() + _tags(u) + b"\n" for i, (u, s) in enumerate(zip(ans["utg"].tolist(), seqs))]
    out += [b"L\tutg%d\t%c\tutg%d\t%c\t%dM\n" % (x, b"+-"[xo], y, b"+-"[yo], o) for x, xo, y, yo, o in ans["links"].tolist()]
    out += [b"L\tutg%d\t+\tutg%d\t+\t%dM\n" % (i, i, u[3]) for i, u in enumerate(ans["utg"].tolist()) if u[3]]
    return b"".join(out)


def table(ans, pair=False):
    out, at = [], 0
    for i, (h, t, n, circ, ln) in enumerate(ans["utg"].tolist()):
        for r, (v, o, off) in enumerate(ans["mem"][at:at + n].tolist()):
            out.append(b"utg%d\t%d\t%d\t%c\t%d\t%d\n" % (i, r, v >> 1, b"+-"[v & 1], off, o) if pair else b"utg%d\t%d\t%d\t%d\t%d\n" % (i, r, v, off, o))
        at += n
    return b"".join(out)


# ---- inputs ----

CHAINS = (1, 2, 3, 4, 5, 8, 9, 33)


def designed(seed=29, both=False):
    """(sequences, what is where): reads of 60 at MIN_LEN 20, every group on contigs of its own.  Tiled chains of CHAINS reads at step 10 (either side of the powers
    of two of the jumping rounds; a chain of one has no edges); a fork; a circle of 6 reads on a circular 120-mer and one of 2 reads of 90; a periodic read (a chain of
    one with a link to itself); reads at 0, 10, 20, 30, 45, 55, 65, 75 of X + revcomp(X) (on both strands one chain of all 16 rows that is its own mirror image).  On
    one strand only: a chain of 1000 reads at step 7 (one unitig of 7053 symbols), and G[0:60] with G[20:60] (the tail is wholly the overlap and writes nothing; on
    both strands that pair makes the graph asymmetric: `SETS`)"""
    rng = np.random.default_rng(seed)
    g = lambda n: util.random_genome(rng, n)    # noqa: E731
    cat = lambda *x: np.concatenate(x).astype(np.uint8)    # noqa: E731
    seqs, where = [], {}

    def put(name, xs):
        where[name] = list(range(len(seqs), len(seqs) + len(xs)))
        seqs.extend(np.asarray(x, dtype=np.uint8).copy() for x in xs)

    for n in CHAINS:
        G = g(60 + 10 * (n - 1))
        put("chain%d" % n, [G[10 * i:10 * i + 60] for i in range(n)])
    G = g(60)
    put("fork", [G, cat(G[10:], g(10)), cat(G[10:], g(10))])
    C = g(120)
    C2 = cat(C, C)
    put("circle6", [C2[20 * i:20 * i + 60] for i in range(6)])
    C = g(120)
    C2 = cat(C, C)
    put("circle2", [C2[0:90], C2[60:150]])
    put("periodic", [np.tile(g(7), 12)])
    X = g(70)
    P = cat(X, util.revcomp(X))
    put("mirror", [P[s:s + 60] for s in (0, 10, 20, 30, 45, 55, 65, 75)])
    if not both:
        G = g(60 + 7 * 999)
        put("chain1000", [G[7 * i:7 * i + 60] for i in range(1000)])
        G = g(60)
        put("contained", [G, G[20:]])
    return seqs, where


def contained_pair(seed=31):
    G = util.random_genome(np.random.default_rng(seed), 60)
    return [G, G[20:].copy()]


# name -> (sequences, both strands, n_asym expected with pair; None: one strand, no symmetry asked)
def SETS():
    return {
        "designed1": (designed(both=False)[0], False),
        "designed2": (designed(both=True)[0], True),
        "reads1": (rm.read_set(), False),
        "reads2": (rm.read_set(), True),
        "contained1": (contained_pair(), False),
        "contained2": (contained_pair(), True),
        "reduce1": (rm.designed_reduce(both=False), False),
        "reduce2": (rm.designed_reduce(both=True), True),
    }


ASYM = {"contained2": 1, "reduce2": 2}
L = MIN_LEN
