"""Host model of the merge's rebuild (k_reb_group, k_plane_group and the placement behind them), numpy only, and the table of
exact insertions that aims at their borders.

The seam: rb3gpu_sh_finish inserts row r (symbol sym[r]) before old position ka[r] for ANY non-decreasing ka[] and rebuilds the index
through build_index, so with from_plain for the old index a test decides what every group kernel sees.

insert()       the reference: merged[ka[r] + r] = sym[r], old symbols in order (fm-index.c:237-249); rows that share an insertion
               point (a TIE) stay in row order.
group_facts()  per output group of 8192 symbols, what reb_group_one<RMAX, NBMAX> decides on, derived from (old, ka, sym) and the slot
               partition of layout_model alone -- and what k_plane_group's word loop meets in that group.
tier()         which kernel ends up with the group: 1 = reb_group_one<384,128>, 2 = <624,320>, 3 = handed on to the symbol path.
cases()        the seeded table (name, old, ka, sym, borders); BORDERS names every border and the predicate on the facts that says a
               case really sits on that side of it (tests/test_cpu_rebuild.py holds the table to it).
second_step()  a fixed mixed insertion applied on top of every case's result: the next rebuild reads the slots the first one wrote."""
import functools

import numpy as np

from tests import layout_model as lm

GRP, WIN = lm.GRP, lm.WIN
T1_SLOTS, T1_ROWS = 384 // lm.RLE_CODES, 128     # reb_group_one<384,128>: old slots of the range, differing rows
T2_SLOTS, T2_ROWS = 624 // lm.RLE_CODES, 320     # reb_group_one<624,320>
MAX_NEW_SLOTS = 8                                # RB3_RG_MAXSLOTS
MAX_GROUP_ROWS = GRP - 64
T1_ROWS_PER_GROUP = 96                           # tune reb_t1_rows: the small tier runs where a group receives at most this many rows on average


def insert(old, ka, sym):
    """old with sym[r] inserted before old[ka[r]] (ka non-decreasing; ties in row order)"""
    old, ka, sym = np.asarray(old, dtype=np.uint8), np.asarray(ka, dtype=np.int64), np.asarray(sym, dtype=np.uint8)
    assert ka.size == sym.size and (ka.size == 0 or (ka[0] >= 0 and ka[-1] <= old.size and (np.diff(ka) >= 0).all()))
    out = np.empty(old.size + ka.size, dtype=np.uint8)
    isrow = np.zeros(out.size, dtype=bool)
    pos = ka + np.arange(ka.size, dtype=np.int64)
    isrow[pos] = True
    out[pos] = sym
    out[~isrow] = old
    return out


def runs_of(plain):
    """the maximal runs of a plain sequence as export_runs() gives them: [(symbol, length)]"""
    b = np.asarray(plain, dtype=np.uint8)
    if b.size == 0:
        return []
    st = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    ln = np.diff(np.concatenate([st, [b.size]]))
    return [(int(c), int(l)) for c, l in zip(b[st], ln)]


def _slot_tables(plain):
    """(slot number of every window, windows of every slot) of the block array of a plain sequence"""
    masks = lm.slot_masks(plain)
    nwin = lm.n_windows(np.asarray(plain).size)
    start = ((masks[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)[:nwin]
    sid = np.cumsum(start) - 1
    return sid, np.bincount(sid), start


def group_facts(old, ka, sym):
    """one dict per output group, see the module text; "ties" lists the group's insertion points as
    (first row in the group, rows, k - A0, offset of the first row that is not absorbed or -1, strictly inside an old run)"""
    old, ka, sym = np.asarray(old, dtype=np.uint8), np.asarray(ka, dtype=np.int64), np.asarray(sym, dtype=np.uint8)
    n, m = old.size, ka.size
    ntot = n + m
    pos = ka + np.arange(m, dtype=np.int64)
    merged = insert(old, ka, sym)
    isrow = np.zeros(lm.n_groups(ntot) * GRP, dtype=bool)
    isrow[pos] = True
    sid, ssize, sstart = _slot_tables(old)
    new_masks = lm.slot_masks(merged)
    # k is strictly inside a CODED run: not the first symbol of the index, of a maximal run, or of a slot
    coded_inside = np.zeros(n + 1, dtype=bool)
    if n > 1:
        coded_inside[1:n] = old[1:] == old[:-1]
    wst = np.flatnonzero(sstart) << lm.WIN_BITS
    coded_inside[wst[wst <= n]] = False
    out = []
    for g in range(lm.n_groups(ntot)):
        P0 = g * GRP
        nsg = min(GRP, ntot - P0)
        j0, j1 = int(np.searchsorted(pos, P0)), int(np.searchsorted(pos, P0 + GRP))
        nb, A0 = j1 - j0, P0 - j0
        nold = nsg - nb
        f = {"g": g, "last": g == lm.n_groups(ntot) - 1, "nsg": nsg, "nb": nb, "A0": A0, "nold": nold, "ns": 0, "n_single": 0,
             "new_slots": bin(int(new_masks[g])).count("1")}
        if nold > 0:
            sa, sb = sid[A0 >> lm.WIN_BITS], sid[(A0 + nold - 1) >> lm.WIN_BITS]
            f["ns"] = int(sb - sa + 1)
            f["n_single"] = int((ssize[sa:sb + 1] == 1).sum())
            f["nw"] = ((A0 + nold - 1) >> 5) - (A0 >> 5) + 1
        else:
            f["nw"] = 0
        # the streamed row pass: a row is absorbed iff it is strictly inside a coded run of its own symbol and no earlier row at
        # the same k was not; the run resumes (a C item) behind the last row of a k that lies inside a run and has an item
        k = ka[j0:j1] - A0
        kabs = ka[j0:j1]
        inside = (k > 0) & (k < nold) & coded_inside[np.minimum(kabs, n)]
        own = np.zeros(nb, dtype=bool)
        own[inside] = sym[j0:j1][inside] == old[kabs[inside]]
        bad = ~own
        khead = np.ones(nb, dtype=bool)
        khead[1:] = k[1:] != k[:-1]
        hidx = np.maximum.accumulate(np.where(khead, np.arange(nb), 0)) if nb else np.zeros(0, dtype=np.int64)
        cb = np.cumsum(bad)
        item = (cb - (cb[hidx] - bad[hidx])) > 0 if nb else np.zeros(0, dtype=bool)
        kend = np.ones(nb, dtype=bool)
        kend[:-1] = k[1:] != k[:-1]
        f["nB"], f["nC"] = int(item.sum()), int((kend & inside & item).sum())
        ties = []
        hs = np.flatnonzero(khead)
        for a, b in zip(hs, np.concatenate([hs[1:], [nb]])):
            fb = np.flatnonzero(bad[a:b])
            ties.append((int(a), int(b - a), int(k[a]), int(fb[0]) if fb.size else -1, bool(inside[a])))
        f["ties"] = ties
        # k_plane_group: one lane per 32 output symbols
        rw = isrow[P0:P0 + GRP].reshape(256, 32)
        cnt = rw.sum(axis=1)
        before = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        wofs = np.arange(256) * 32
        nval = np.clip(nsg - wofs, 0, 32)
        takes_old = (nval - cnt) > 0
        f["shifts"] = set(((A0 + wofs - before) & 31)[takes_old].tolist())
        f["row_words"] = int(((cnt == 32) & (nval == 32)).sum())
        out.append(f)
    return out


def tier(f, t1=True):
    """1, 2: the tier of k_reb_group that rebuilds the group; 3: handed on.  t1 False: the small tier does not run"""
    if f["last"] or f["nb"] > MAX_GROUP_ROWS or f["n_single"] > 0 or f["new_slots"] > MAX_NEW_SLOTS:
        return 3
    if t1 and f["ns"] <= T1_SLOTS and f["nB"] <= T1_ROWS:
        return 1
    if f["ns"] <= T2_SLOTS and f["nB"] <= T2_ROWS:
        return 2
    return 3


def why3(f):
    """the reasons a group is handed on by the medium tier"""
    w = []
    if f["last"]: w.append("last")
    if f["nb"] > MAX_GROUP_ROWS: w.append("nb")
    if f["n_single"] > 0: w.append("plane")
    if f["new_slots"] > MAX_NEW_SLOTS: w.append("new_slots")
    if f["ns"] > T2_SLOTS: w.append("ns")
    if f["nB"] > T2_ROWS: w.append("nB")
    return w


def runspace_runs(old, window_rebuild=False, reb_force=1):
    """does build_index start k_reb_group on this old index (runspace_applies with reb_force set)?  Not from a fully bit-plane index"""
    return reb_force > 0 and not window_rebuild and lm.slot_count(old) != lm.n_windows(np.asarray(old).size)


def hand_over(old, ka, sym, t1_rows=T1_ROWS_PER_GROUP, facts=None):
    """(groups seen by the run-space rebuild, groups the small tier hands to the medium one, groups handed on to the symbol path) of one
    rebuild under reb_force 1: the growth of n_reb_groups, n_reb_groups_tier2 and n_reb_groups_window"""
    if not runspace_runs(old):
        return 0, 0, 0
    facts = facts if facts is not None else group_facts(old, ka, sym)
    ntot = np.asarray(old).size + np.asarray(ka).size
    t1 = float(np.asarray(ka).size) * GRP / float(max(ntot, 1)) <= float(t1_rows)
    ts = [tier(f, t1) for f in facts]
    return len(facts), (sum(t >= 2 for t in ts) if t1 else 0), sum(t == 3 for t in ts)


def row_runs(ka):
    """maximal stretches of consecutive merged positions that are all rows: [(first merged position, rows)]"""
    ka = np.asarray(ka, dtype=np.int64)
    if ka.size == 0:
        return []
    pos = ka + np.arange(ka.size)
    st = np.flatnonzero(np.concatenate([[True], np.diff(pos) != 1]))
    return [(int(pos[a]), int(b - a)) for a, b in zip(st, np.concatenate([st[1:], [ka.size]]))]


def second_step(n):
    """about 300 rows into an index of n symbols: all six symbols, single rows and ties of up to 40 rows, ka = 0 and ka = n included"""
    rng = np.random.default_rng(20261020)
    u = np.sort(rng.random(300))
    for a, l in ((20, 3), (90, 40), (200, 9), (260, 2)):
        u[a:a + l] = u[a]
    ka = np.minimum((u * (n + 1)).astype(np.int64), n)
    ka[0], ka[-1] = 0, n
    return ka, rng.integers(0, 6, size=300, dtype=np.uint8)


# ---- old indexes ----

def _old_long(rng, n, lo=700, hi=2600, syms=(1, 2, 3, 4)):
    """runs of lo..hi symbols: every whole group is one run slot of 32 windows"""
    parts, tot, prev = [], 0, None
    while tot < n:
        l = int(rng.integers(lo, hi))
        s = int(rng.choice([x for x in syms if x != prev]))
        parts.append(np.full(l, s, dtype=np.uint8))
        tot, prev = tot + l, s
    return np.concatenate(parts)[:n].copy()


def _block(rng, length, nruns, first_not, edge=16):
    """lm._runs_block whose first and last runs are at least `edge` long (a few rows inserted into the block push none of its runs out)"""
    while True:
        p = lm._runs_block(rng, length, nruns, first_not)
        h = np.flatnonzero(np.concatenate([[True], p[1:] != p[:-1]]))
        if h.size == nruns and (nruns == 1 or (h[1] >= edge and length - h[-1] >= edge)):
            return p


def _old_blocks4(rng, ngroups, tail=100):
    """aligned blocks of 4 windows with exactly 40 runs each: 8 run slots per whole group"""
    parts, prev = [], None
    for _ in range(ngroups * 8):
        p = _block(rng, 4 * WIN, 40, prev)
        parts.append(p)
        prev = int(p[-1])
    parts.append(np.full(tail, 1 + prev % 4, dtype=np.uint8))
    return np.concatenate(parts)


def _old_both(rng, ngroups, tail=100):
    """in every group 16 windows of random symbols (bit planes) then 16 windows of long runs (run slots)"""
    parts = []
    for _ in range(ngroups):
        parts.append(rng.integers(0, 6, size=16 * WIN, dtype=np.uint8))
        parts.append(_block(rng, 16 * WIN, 9, None, edge=100))
    parts.append(rng.integers(0, 6, size=tail, dtype=np.uint8))
    return np.concatenate(parts)


def _old_ns13(rng):
    """group 1 is 16 run slots of 2 windows whose run counts make every aligned 4-window block hold 49 runs, while every 4-window block
    that starts 2 windows later holds 47: shifted by 6 windows of absorbed rows, 26 of its windows (13 old slots) become 7 new slots"""
    p = [0] * 16
    for i in range(8):
        p[2 * i] = 46 - 2 * i
    for i in range(7):
        p[2 * i + 1] = 47 - p[2 * i + 2]
    p[15] = 49 - p[14]
    g0 = _old_long(rng, GRP)
    parts, prev = [g0], int(g0[-1])
    for j in range(16):
        b = _block(rng, 2 * WIN, p[j], prev, edge=3)
        parts.append(b)
        prev = int(b[-1])
    rest = _old_long(rng, 2 * GRP + 100, syms=tuple(x for x in (1, 2, 3, 4) if x != prev))
    return np.concatenate(parts + [rest])


def _inside(old):
    """positions strictly inside a maximal run and not on a window start (so inside a coded run whatever the slots are)"""
    ok = np.zeros(old.size + 1, dtype=bool)
    ok[1:old.size] = old[1:] == old[:-1]
    ok[::WIN] = False
    return ok


def _next(mask, k):
    return int(k + np.argmax(mask[k:]))


def _other(s, i=0, pool=(1, 2, 3, 4, 0, 5)):
    return [x for x in pool if x != s][i % 5]


class _Rows:
    """rows collected in increasing ka"""

    def __init__(self, old):
        self.old, self.ka, self.sym = old, [], []
        self.inside = _inside(old)
        self.start = np.zeros(old.size + 1, dtype=bool)
        self.start[1:old.size] = old[1:] != old[:-1]

    def add(self, k, syms):
        syms = list(np.atleast_1d(syms))
        assert not self.ka or k >= self.ka[-1]
        self.ka += [int(k)] * len(syms)
        self.sym += [int(s) for s in syms]

    def absorbed(self, k, count=1, step=2):
        """`count` rows of the run's own symbol at distinct points strictly inside runs, from k on; returns the next free k"""
        for _ in range(count):
            k = _next(self.inside, k)
            self.add(k, self.old[k])
            k += step
        return k

    def arrays(self):
        return np.array(self.ka, dtype=np.int64), np.array(self.sym, dtype=np.uint8)


def _case(name, old, rows, borders):
    ka, sym = rows.arrays() if isinstance(rows, _Rows) else rows
    return (name, old, np.asarray(ka, dtype=np.int64), np.asarray(sym, dtype=np.uint8), tuple(borders))


TIE_ROWS = tuple(range(58, 67)) + tuple(range(122, 131)) + tuple(range(186, 195))
CUT_OFFSETS = (1, 63, 64, 136, 199)
PLANE_RUNS = (31, 32, 33, 64, 255, 256, 257, 300, 8192)
PLANE_OFFS = (0, 1, 31)


def _tier_cases(rng):
    out = []
    long4 = _old_long(rng, 4 * GRP + 100)
    long4[GRP - 50:GRP + 700] = 1     # one run around the start of group 1: what is clustered there stays in its first windows
    ins = _inside(long4)
    # nB 128|129 and 320|321: once as one tie inside a long run, once as distinct k clustered in two windows (a C item behind every row)
    for m in (128, 129, 320, 321):
        k = _next(ins, GRP + 1000)
        s = int(long4[k])
        r = _Rows(long4)
        r.add(k, [_other(s, 0)] * m)
        out.append(_case("tier_nB%d_tie" % m, long4, r, ["nB%d_tie" % m]))
        r = _Rows(long4)
        for i, k in enumerate(np.flatnonzero(ins[:GRP + 690])[np.searchsorted(np.flatnonzero(ins[:GRP + 690]), GRP + 1):][:m]):
            r.add(k, _other(1, i))
        out.append(_case("tier_nB%d_spread" % m, long4, r, ["nB%d_spread" % m]))
    # nb 8128|8129: one tie of the run's own symbol, every row of it in group 1
    for m in (MAX_GROUP_ROWS, MAX_GROUP_ROWS + 1):
        k = _next(ins, GRP + 10)
        r = _Rows(long4)
        r.add(k, [int(long4[k])] * m)
        out.append(_case("tier_nb%d" % m, long4, r, ["nb%d" % m]))
    # ns 8|9: 4-window run slots, one absorbed row: group 1 reads 8 old slots, group 2 (one symbol earlier) 9
    b4 = _old_blocks4(rng, 4)
    r = _Rows(b4)
    r.absorbed(GRP + 3000)
    out.append(_case("tier_ns8_9", b4, r, ["ns8", "ns9"]))
    # new slots 8|9: 4 and 5 differing rows into the last 4-window block (40 runs) of group 1: 48 runs stay one slot, 50 do not;
    # 4 rows and one on a run start: 49
    bins = _inside(b4)
    for m, extra, tag in ((4, 0, "newslots8"), (5, 0, "newslots9"), (4, 1, "runs49")):
        r = _Rows(b4)
        k = GRP + 28 * WIN + 40
        for i in range(m):
            k = _next(bins & np.concatenate([bins[1:], [False]]), k)   # the run goes on for two more symbols
            r.add(k, _other(int(b4[k]), i))
            k += 150
        if extra:
            k = _next(r.start, k)
            r.add(k, [x for x in (1, 2, 3, 4, 5) if x != b4[k] and x != b4[k - 1]][0])
        out.append(_case("tier_" + tag, b4, r, [tag]))
    # ns 13|14
    o13 = _old_ns13(rng)
    s = int(o13[GRP])
    assert o13[GRP + 1] == s
    r = _Rows(o13)
    r.add(GRP + 1, [s] * (6 * WIN))
    out.append(_case("tier_ns13", o13, r, ["ns13"]))
    r = _Rows(o13)
    r.absorbed(4000)
    r.add(GRP + 1, [s] * (6 * WIN))
    out.append(_case("tier_ns14", o13, r, ["ns14"]))
    # one bit-plane slot in the old range of a group of run slots
    op = long4.copy()
    op[GRP + 5 * WIN:GRP + 6 * WIN] = rng.integers(0, 6, size=WIN, dtype=np.uint8)
    r = _Rows(op)
    r.absorbed(GRP + 200)
    r.add(_next(_inside(op), GRP + 7 * WIN), 5)
    out.append(_case("tier_plane_slot_in_range", op, r, ["plane_in_range"]))
    # the last group with 0, 1, 255, 256 and 257 symbols
    for left in (0, 1, 255, 256, 257):
        o = _old_long(rng, 3 * GRP + left - 6)
        r = _Rows(o)
        k = r.absorbed(GRP + 77, 3)
        r.add(_next(_inside(o), 2 * GRP + 500), [_other(int(o[_next(_inside(o), 2 * GRP + 500)]), 1)] * 2)
        r.add(o.size, 2)
        out.append(_case("tier_last%d" % left, o, r, ["last%d" % left]))
    return out


def _tie_cases(rng):
    out = []
    old = _old_long(rng, 4 * GRP + 100, 200, 500)
    for s in range(9):
        for d0 in (0, 3, 6):
            for onstart in (False, True):
                r = _Rows(old)
                tags = []
                k = _next(r.inside, 500 + 7 * s)     # (a lone differing row in group 0: moving it is seen whatever the ties absorb)
                r.add(k, _other(int(old[k]), d0))
                for gi in (1, 2, 3):
                    D = d0 + gi - 1          # the first differing row of the group's ties; 8: none differs
                    k = gi * GRP - len(r.ka) + 300
                    for t in range(3):
                        k = r.absorbed(k, 58 + s if t == 0 else 56)
                        k = _next(r.start if onstart else r.inside, k + 1)
                        rs = int(old[k])
                        x, y = _other(rs, s + t), _other(rs, s + t + 2)
                        pat = [x, rs, y, y, rs, x, rs, y]
                        r.add(k, [rs] * min(D, 8) + pat[:max(8 - D, 0)])
                        tags.append("tie_r%d_d%d_%s" % (58 + s + 64 * t, D, "start" if onstart else "inside"))
                        k += 2
                out.append(_case("tie_s%d_d%d_%s" % (s, d0, "start" if onstart else "inside"), old, r, tags))
    # a tie of 200 rows cut by the border between groups 1 and 2
    oc = old.copy()
    oc[2 * GRP - 400:2 * GRP + 400] = 3
    for off in CUT_OFFSETS:
        for differ in (False, True):
            r = _Rows(oc)
            k = r.absorbed(GRP + 100, 5)
            syms = [3] * 200 if not differ else [(1, 2, 3, 4, 0, 5, 3)[i % 7] for i in range(200)]
            r.add(2 * GRP - off - len(r.ka), syms)
            out.append(_case("tie200_cut%d_%s" % (off, "differ" if differ else "own"), oc, r, ["cut%d_%s" % (off, "differ" if differ else "own")]))
    return out


def _geometry_cases(rng):
    out = []
    old = _old_long(rng, 4 * GRP + 100, 300, 900)
    base = _Rows(old)
    # a row on a maximal run start with the symbol of the run before, of the run after, of neither
    r = _Rows(old)
    k = GRP + 500
    for which in range(3):
        k = _next(r.start, k)
        r.add(k, [int(old[k - 1]), int(old[k]), [x for x in (1, 2, 3, 4, 5) if x != old[k] and x != old[k - 1]][0]][which])
        k += 700
    out.append(_case("geo_row_on_run_start", old, r, ["run_start_before", "run_start_after", "run_start_neither"]))
    # a row on a slot border inside a run (the border between two old groups), own symbol and another
    ob = old.copy()
    ob[2 * GRP - 200:2 * GRP + 200] = 2
    for s in (2, 4):
        r = _Rows(ob)
        r.add(2 * GRP, s)
        out.append(_case("geo_slot_border_in_run_%s" % ("sym4" if s == 4 else "own"), ob, r, ["slot_border_in_run"]))
    r = _Rows(ob)
    r.add(_next(r.inside, GRP + 300), 0)
    r.add(2 * GRP, [2, 2, 1, 2])
    out.append(_case("geo_slot_border_in_run_tie", ob, r, ["slot_border_in_run"]))
    # rows at ka = 0 and ka = n, symbols 0 and 5
    r = _Rows(old)
    r.add(0, [0, int(old[0]), 5])
    r.add(_next(base.inside, GRP + 9), [5, 0])
    r.add(old.size, [int(old[-1]), 5, 0])
    out.append(_case("geo_first_and_last_position_sym0_sym5", old, r, ["ka0", "kan", "sym0", "sym5"]))
    # an old run over 3 whole groups, rows in the middle group only
    o3 = np.concatenate([_old_long(rng, 5000, 300, 900), np.full(3 * GRP + 6000, 3, dtype=np.uint8), _old_long(rng, 2000, 300, 900, syms=(1, 2, 4))])
    r = _Rows(o3)
    r.add(2 * GRP + 100, 3)
    r.add(2 * GRP + 1000, [1, 3, 3])
    r.add(2 * GRP + 1001, 3)
    r.add(2 * GRP + 4096, 2)
    r.add(2 * GRP + 8000, [3] * 70)
    out.append(_case("geo_run_over_three_groups", o3, r, ["run_over_groups"]))
    # totals that stay below, land on and cross a multiple of 8192 and of 256
    for mult, n0 in ((GRP, 3 * GRP - 5), (WIN, 2 * GRP + 3 * WIN - 5)):
        o = _old_long(rng, n0, 300, 900)
        for m in (3, 5, 8):
            r = _Rows(o)
            k = _next(_inside(o), GRP + 50)
            r.add(k, [_other(int(o[k]), m)] * (m - 1))
            r.add(o.size, 1 + m % 4)
            out.append(_case("geo_total_%d_%+d" % (mult, m - 5), o, r, ["total_%d_%s" % (mult, ("below", "on", "across")[(3, 5, 8).index(m)])]))
    # one row
    for k, s in ((_next(base.inside, GRP + 4000), 0), (_next(base.start, 2 * GRP + 10), 5)):
        r = _Rows(old)
        r.add(k, s)
        out.append(_case("geo_one_row_k%d" % k, old, r, ["n_rows_1"]))
    # heads exactly on window starts: runs of 512 symbols; a differing row in the middle of group 1 moves the later ones off them
    ow = np.concatenate([np.full(2 * WIN, 1 + i % 4, dtype=np.uint8) for i in range(66)])
    r = _Rows(ow)
    r.add(GRP + 4000, 5)
    r.add(3 * GRP + 512, 0)   # exactly on a head that is a window start
    out.append(_case("geo_heads_on_window_starts", ow, r, ["wexact"]))
    return out


def _plane_cases(rng):
    out = []
    olds = {"dense": rng.integers(0, 6, size=4 * GRP + 100, dtype=np.uint8), "runs": _old_long(rng, 4 * GRP + 100, 300, 900), "both": _old_both(rng, 4)}
    i = 0
    for L in PLANE_RUNS:
        for off in PLANE_OFFS:
            kind = ("dense", "runs", "both")[i % 3]
            pre = (i // 3) % 2      # one row in group 0: the old range of group 1 starts at A0 & 31 == 31
            i += 1
            old = olds[kind]
            r = _Rows(old)
            if pre:
                r.add(100, int(old[100]) ^ 1)
            start = GRP + off if L == GRP else GRP + 32 * 5 + off
            r.add(start - pre, rng.integers(0, 6, size=L, dtype=np.uint8))
            out.append(_case("plane_run%d_off%d_%s_pre%d" % (L, off, kind, pre), old, r, ["rowrun%d_off%d" % (L, off)]))
    # rows scattered one per word, then every other symbol a row: shifts 0..31 and masks of every density
    for kind in ("dense", "runs", "both"):
        old = olds[kind]
        r = _Rows(old)
        for k in range(GRP, GRP + 2000, 31):
            r.add(k, int(rng.integers(0, 6)))
        for k in range(2 * GRP, 2 * GRP + 1500):
            r.add(k, int(rng.integers(0, 6)))
        out.append(_case("plane_scattered_" + kind, old, r, ["old_" + kind]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """the table (name, old, ka, sym, borders); seeded, the same on every call.  Old indexes hold at most 5 groups"""
    rng = np.random.default_rng(20261021)
    out = _tier_cases(rng) + _tie_cases(rng) + _geometry_cases(rng) + _plane_cases(rng)
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        for a in c[1:4]:
            a.setflags(write=False)
    return tuple(out)


def kind_of(name):
    return name.split("_")[0]   # tier, tie / tie200, geo, plane


# ---- the borders: tag -> predicate on (facts of the case, the case) ----

def _only(f, reason):
    return why3(f) == [reason]


def _grp(facts, pred):
    return any(pred(f) for f in facts)


def _tie_pred(row, d, onstart):
    def p(facts, case):
        for f in facts:
            for (a, l, k, fb, inside) in f["ties"]:
                if a == row and l == 8 and inside != onstart and 0 < k < f["nold"]:
                    if onstart and fb == 0:
                        return True     # every row of a tie on a run start is an item
                    if not onstart and fb == (d if d < 8 else -1):
                        return True
        return False
    return p


def _cut_pred(off, differ):
    def p(facts, case):
        for f, fn in zip(facts[:-1], facts[1:]):
            if f["ties"] and fn["ties"]:
                a, l, k, fb, _ = f["ties"][-1]
                a2, l2, k2, _, _ = fn["ties"][0]
                sy = case[3]
                j0 = sum(x["nb"] for x in facts[:f["g"]])
                own = bool((sy[j0 + a:j0 + a + 200] == case[1][case[2][j0 + a]]).all())
                if l == off and l2 == 200 - off and k == f["nold"] and k2 == 0 and a2 == 0 and own != differ:
                    return True
        return False
    return p


def _rowrun_pred(L, off):
    return lambda facts, case: any(l == L and p % 32 == off for p, l in row_runs(case[2]))


def _build_borders():
    B = {}
    within1 = lambda f: not f["last"] and f["nb"] <= MAX_GROUP_ROWS and f["n_single"] == 0 and f["new_slots"] <= MAX_NEW_SLOTS
    B["ns8"] = lambda F, c: _grp(F, lambda f: f["ns"] == 8 and tier(f) == 1)
    B["ns9"] = lambda F, c: _grp(F, lambda f: f["ns"] == 9 and f["nB"] <= T1_ROWS and tier(f) == 2)
    B["ns13"] = lambda F, c: _grp(F, lambda f: f["ns"] == 13 and tier(f) == 2)
    B["ns14"] = lambda F, c: _grp(F, lambda f: f["ns"] == 14 and _only(f, "ns"))
    for m, t in ((128, 1), (129, 2), (320, 2), (321, 3)):
        B["nB%d_tie" % m] = (lambda m, t: lambda F, c: _grp(F, lambda f: f["nB"] == m and len(f["ties"]) == 1 and f["ns"] <= T1_SLOTS and within1(f) and tier(f) == t))(m, t)
        B["nB%d_spread" % m] = (lambda m, t: lambda F, c: _grp(F, lambda f: f["nB"] == m and f["nC"] == m and len(f["ties"]) == m and f["ns"] <= T1_SLOTS and within1(f) and tier(f) == t))(m, t)
    B["newslots8"] = lambda F, c: _grp(F, lambda f: f["new_slots"] == 8 and 0 < f["nB"] and tier(f) == 1)
    B["newslots9"] = lambda F, c: _grp(F, lambda f: f["new_slots"] == 9 and _only(f, "new_slots") and f["ns"] <= T1_SLOTS and f["nB"] <= T1_ROWS)
    B["runs49"] = B["newslots9"]
    B["nb8128"] = lambda F, c: _grp(F, lambda f: f["nb"] == MAX_GROUP_ROWS and tier(f) == 1)
    B["nb8129"] = lambda F, c: _grp(F, lambda f: f["nb"] == MAX_GROUP_ROWS + 1 and _only(f, "nb"))
    # (a single window never stands alone in a whole group: the window it shares a block of two with is single too)
    B["plane_in_range"] = lambda F, c: _grp(F, lambda f: 0 < f["n_single"] < f["ns"] and _only(f, "plane"))
    for left in (0, 1, 255, 256, 257):
        B["last%d" % left] = (lambda left: lambda F, c: F[-1]["last"] and F[-1]["nsg"] == left)(left)
    for row in TIE_ROWS:
        for d in range(9):
            B["tie_r%d_d%d_inside" % (row, d)] = _tie_pred(row, d, False)
            B["tie_r%d_d%d_start" % (row, d)] = _tie_pred(row, d, True)
    for off in CUT_OFFSETS:
        B["cut%d_own" % off] = _cut_pred(off, False)
        B["cut%d_differ" % off] = _cut_pred(off, True)
    for L in PLANE_RUNS:
        for off in PLANE_OFFS:
            B["rowrun%d_off%d" % (L, off)] = _rowrun_pred(L, off)
    # the planes list, met somewhere in the table (PLANE_FACTS below): checked over all cases together
    return B


BORDERS = _build_borders()

# facts of k_plane_group that some group of some case must show: name -> predicate on one group's facts
PLANE_FACTS = {
    "a0_0": lambda f: f["nb"] > 0 and f["nold"] > 0 and f["A0"] & 31 == 0,
    "a0_31": lambda f: f["nb"] > 0 and f["nold"] > 0 and f["A0"] & 31 == 31,
    "word_of_rows_only": lambda f: f["row_words"] > 0,
    "shift0": lambda f: 0 in f["shifts"],
    "shift31": lambda f: 31 in f["shifts"],
    "rows256": lambda f: f["nb"] == 256,
    "rows257": lambda f: f["nb"] == 257,
    "rows_only_group": lambda f: f["nsg"] == GRP and f["nold"] == 0,
    "old_words257": lambda f: f["nw"] == 257,
    "old_dense": lambda f: f["nb"] > 0 and f["ns"] > 0 and f["n_single"] == f["ns"],
    "old_runs": lambda f: f["nb"] > 0 and f["ns"] > 0 and f["n_single"] == 0,
    "old_both": lambda f: f["nb"] > 0 and 0 < f["n_single"] < f["ns"],
}

# borders of the issue's list that no input reaches, with the reason
UNREACHABLE = {
    "old_words258": "the old range of a group is at most 8192 symbols from an offset of at most 31 in its first word: ((31 + 8192 - 1) >> 5) + 1 = 257 words "
                    "(PgLds.opl has room for 264)",
}
