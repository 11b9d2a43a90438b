"""Host model of the merge's settle phase (k_events, k_cum, k_resolve_w, k_sfin, k_wj_*, their wide-mask twins and k_resolve),
plain Python and numpy, no popcount or select tricks -- and the table of hand-made stretch tables that aims at their borders.

A scenario says what happened, not how it is stored:
  W(K, d0, ...)  a walker whose first interval has K rows, d0 of which (0 <= d0 <= K) lie below the new suffix: the true unknown
                 of its first stretch.  events: per drop-out event, the SURVIVOR indices that dropped (what k_events leaves: bit i
                 <=> the i-th row of the interval as it was then), or ("ix", lo, c): the rows of [lo, lo + survivors) of the
                 scenario's index that do not hold c.  dels: the stretches (0 = the first) that a better-informed walker
                 settled: del = 1 + the TRUE unknown, as an exact walker leaves it.  link = (walker, stretch, offset[, "lost"]):
                 the walker ran into a tentative record of that stretch of another walker, offset = lo_A - lo_B, d_B = d_A + offset;
                 "lost": another follower's link into the same stretch was written later.
The truth is by construction: d_t = #{survivors after event t whose original index < d0}.  build() refuses a scenario whose links
or intervals contradict it, and anything that would take a kernel outside the table or the index.

The encoder restates what k_chain writes (csrc/rb3gpu_kernels.h):
  an event (the `ew0`/`ew1` lines and the three stores of evq_flush / the general step): tab[ns].w0 = EVENT << 62 | sid << 38 | lo,
      .w1 = kk | c << 16 | tp << 20, tab[ns].pad[0] = sid0 + 1, tab[sid].child = ns + 1;
  ids ("ns = sid + 1 ... (ns & (RB3_TENT_CHUNK - 1)) == 0 -> tent_take_chunk", and the first record's `gap == 1 ? atomicAdd(sidctr + 1, 1u)`):
      a walker of more than one row takes aligned blocks of 8 ids from the lower half, chunk n of counter c = ids [(n * 64 + c) * 8, + 8),
      its next chunk at a higher id; a walker of one row takes a single id from RB3_TENT_HALF up; ids nobody took stay zero;
  a settled unknown (`tab[sid].del = 1 + (int)(seen - myval)`, `tab[id2].del = 1 + (int)diff`): del = 1 + d;
  a link (`tab[id2].w0 = RB3_DEP_W0(RB3_DEP_LINK, sid, 0), tab[id2].w1 = (uint32)diff, tab[sid].child = id2 + 1`) -- into ANY stretch
      id2, so one written into an event stretch replaces that event's w0 / w1.

cases() is the table, BORDERS one predicate per border (tests/test_cpu_settle.py holds the table to them)."""
import functools

import numpy as np

from tests import layout_model as lm

IDS, HALF, BLOCK, NCTR, CHUNK, PBITS = 1 << 24, 1 << 23, 8, 64, 8, 38
EVENT, LINK = 1, 2
RESW_MAXHOPS = 64     # RB3_RESW_MAXHOPS: what merge_core passes; the staged path passes RB3_TENT_IDS
U32 = 0xFFFFFFFF


class W:
    def __init__(self, K, d0, events=(), dels=(), link=None, far=0):
        self.K, self.d0, self.events, self.dels, self.link, self.far = K, d0, list(events), tuple(dels), link, far


class Case:
    def __init__(self, name, walkers, tags, kind="complete", must=None, must_v1=None, q=1, plain=None):
        self.name, self.walkers, self.tags, self.kind, self.q, self.plain = name, walkers, tuple(tags), kind, q, plain
        self.must, self.must_v1 = must, must_v1   # lists of (walker, stretch); complete cases: everything (must_v1: what k_resolve owes instead)


def bits(idx):
    m = 0
    for i in idx:
        m |= 1 << int(i)
    return m


def words(m, nw):
    return [(m >> (32 * i)) & U32 for i in range(nw)]


class Table:
    """what build() makes of a case: the records, and everything a test may ask about them"""


def build(case):
    q, T = case.q, Table()
    kmax = 256 * q - 1
    ws = case.walkers
    plain = None if case.plain is None else np.asarray(case.plain, dtype=np.uint8)
    # ---- the truth, walker by walker
    T.surv, T.d, T.evmask, T.cum, T.evrec = [], [], [], [], []
    for w in ws:
        assert 1 <= w.K <= kmax and 0 <= w.d0 <= w.K, "interval or unknown out of range"
        assert w.K > 1 or not w.events, "a walker of one row never sees a drop-out"
        surv, d, evm, cum, evr, acc = [list(range(w.K))], [w.d0], [0], [0], [None], 0
        for e in w.events:
            cur = surv[-1]
            if isinstance(e, tuple) and e and e[0] == "ix":
                lo, c = int(e[1]), int(e[2])
                assert plain is not None and 0 <= lo and lo + len(cur) <= plain.size, "interval outside the index"
                drop = [i for i in range(len(cur)) if int(plain[lo + i]) != c]
                evr.append((lo, c))
            else:
                drop = sorted(set(int(i) for i in e))
                evr.append((0, 0))
            assert drop and 0 <= drop[0] and drop[-1] < len(cur) and 1 <= len(cur) - len(drop), "an event drops some rows, never all (1 <= kn < kq)"
            gone = set(drop)
            acc |= bits(cur[i] for i in drop)
            surv.append([r for i, r in enumerate(cur) if i not in gone])
            d.append(sum(1 for r in surv[-1] if r < w.d0))
            evm.append(bits(drop))
            cum.append(acc)
        T.surv.append(surv), T.d.append(d), T.evmask.append(evm), T.cum.append(cum), T.evrec.append(evr)
    # ---- ids: first chunks in walker order, then the continuation chunks (a walker's next chunk lies behind other walkers' blocks)
    T.sid, chunk, singles = {}, 0, 0
    for wi, w in enumerate(ws):
        if w.K == 1:
            T.sid[(wi, 0)] = HALF + singles
            singles += 1
        else:
            for t in range(min(BLOCK, len(T.d[wi]))):
                T.sid[(wi, t)] = chunk * CHUNK + t
            chunk += 1
    for wi, w in enumerate(ws):
        for t in range(BLOCK, len(T.d[wi])):
            if t % BLOCK == 0:
                chunk += w.far     # chunks other waves took and never used: zero ids in between
                base, chunk = chunk * CHUNK, chunk + 1
            T.sid[(wi, t)] = base + t % BLOCK
    T.ctr = np.array([(chunk - c + NCTR - 1) // NCTR if chunk > c else 0 for c in range(NCTR)], dtype=np.uint32)
    T.n_a, T.n_b = chunk * CHUNK, singles
    T.n_a_fused = int(T.ctr.max()) * NCTR * CHUNK     # k_tent_extent: the largest counter, not the last chunk
    assert T.n_a_fused <= HALF and T.n_b < HALF - 1
    # ---- the records
    rec = {s: dict(w0=0, w1=0, dl=0, child=0, mask=0, pad0=0) for s in T.sid.values()}
    T.overwritten, T.first, T.last = set(), [T.sid[(wi, 0)] for wi in range(len(ws))], [T.sid[(wi, len(T.d[wi]) - 1)] for wi in range(len(ws))]
    for wi, w in enumerate(ws):
        for t in range(1, len(T.d[wi])):
            s, p = T.sid[(wi, t)], T.sid[(wi, t - 1)]
            lo, c = T.evrec[wi][t]
            rec[s].update(w0=EVENT << 62 | p << PBITS | lo, w1=len(T.surv[wi][t - 1]) | c << 16 | (1000 + t) << 20, pad0=T.first[wi] + 1, mask=T.evmask[wi][t])
            rec[p]["child"] = s + 1
        for t in w.dels:
            rec[T.sid[(wi, t)]]["dl"] = 1 + T.d[wi][t]
    won = {}
    for wi, w in enumerate(ws):
        if w.link is None:
            continue
        wj, t, off = w.link[:3]
        assert wj != wi and (wj, t) in T.sid, "a link names a stretch of another walker"
        assert T.d[wj][t] == T.d[wi][-1] + off, "the link contradicts the truth: d_B = d_A + offset"
        tgt = T.sid[(wj, t)]
        rec[T.last[wi]]["child"] = tgt + 1
        if len(w.link) > 3 and w.link[3] == "lost":
            continue
        assert tgt not in won, "two links into one stretch: one of them is lost"
        won[tgt] = wi
        rec[tgt].update(w0=LINK << 62 | T.last[wi] << PBITS, w1=off & U32)
        if t > 0:
            rec[tgt]["mask"] = 0     # k_events never saw the event
            T.overwritten.add(tgt)
    T.won = won
    T.ids = np.array(sorted(rec), dtype=np.int32)
    T.rec = np.zeros((T.ids.size, 16), dtype=np.uint32)
    T.ev = np.zeros((T.ids.size, 8 * q), dtype=np.uint32)     # the per-event masks as k_events[_x] leaves them
    for i, s in enumerate(T.ids.tolist()):
        r = rec[s]
        m8 = words(r["mask"], 8 * q)
        T.ev[i] = m8
        T.rec[i] = [r["w0"] & U32, r["w0"] >> 32, r["w1"] & U32, r["w1"] >> 32, r["dl"], r["child"]] + (m8 if q == 1 else [0] * 8) + [r["pad0"], 0]
    T.row = {s: i for i, s in enumerate(T.ids.tolist())}
    # every index a kernel follows stays inside [0, n_a) and [HALF, HALF + n_b)
    inside = lambda s: 0 <= s < T.n_a or HALF <= s < HALF + T.n_b
    for r in rec.values():
        named = ([(r["w0"] >> PBITS) & (IDS - 1)] if r["w0"] >> 62 else []) + [r[k] - 1 for k in ("child", "pad0") if r[k]]
        assert all(inside(x) for x in named), "a record names an id outside the extents"
    # ---- what the tests ask
    T.truth = {T.sid[(wi, t)]: T.d[wi][t] for wi in range(len(ws)) for t in range(len(T.d[wi]))}
    T.width = {T.sid[(wi, t)]: len(T.surv[wi][t]) for wi in range(len(ws)) for t in range(len(T.d[wi]))}
    T.reached = {}     # event stretches k_cum reaches -> their cumulative mask; first stretches of walkers with blocks that have a child -> the last one reached
    for wi, w in enumerate(ws):
        if w.K == 1:
            continue
        last = 0
        for t in range(1, len(T.d[wi])):
            if T.sid[(wi, t)] in T.overwritten:
                break
            T.reached[T.sid[(wi, t)]] = T.cum[wi][t]
            last = t
        if rec[T.first[wi]]["child"]:
            T.reached[T.first[wi]] = T.cum[wi][last]
    everything = [k for k in T.sid]
    named = lambda ks: [k for k in everything if k in ks or (k[0], None) in ks]     # (walker, None): every stretch of that walker
    T.must = {T.sid[k] for k in (everything if case.kind == "complete" else named(set(case.must)))}
    T.must_v1 = T.must if case.must_v1 is None else {T.sid[k] for k in named(set(case.must_v1))}
    assert T.must
    # walkers on the longest dependency path k_resolve_w follows: from a first stretch somebody settled over links into FIRST stretches nobody settled
    nxt = {won[T.first[wj]]: wj for wj in range(len(ws)) if T.first[wj] in won and 0 not in ws[wj].dels}
    T.path = 0
    for wi, w in enumerate(ws):
        if w.dels:
            n, x = 1, wi
            while x in nxt and not any(T.sid[(x, t)] in T.overwritten for t in range(len(T.d[x]))):
                x, n = nxt[x], n + 1
            T.path = max(T.path, n)
    return T


def second_chance(T, maxhops):
    """k_resolve_w settles the first maxhops + 1 walkers of a path and counts in bad[2] when there is one more"""
    return T.path > maxhops + 1


def check(T, case, sfin, engine=0):
    """the asserts of the GPU test on the unknowns of one run: soundness everywhere, completeness on the must-settle set"""
    wrong = [(int(s), int(v) - 1, T.truth[int(s)]) for s, v in zip(T.ids, sfin) if v != 0 and v != 1 + T.truth[int(s)]]
    assert not wrong, "%s: settled to a wrong value (id, sfin - 1, truth): %s" % (case.name, wrong[:8])
    need = T.must_v1 if engine == 1 else T.must
    miss = [s for s in sorted(need) if sfin[T.row[s]] == 0]
    assert not miss, "%s: left unsettled: %s" % (case.name, miss[:8])


def decode(T):
    """records -> fields, the way the kernels read them (the round trip of the encoder)"""
    out = {}
    for s, r in zip(T.ids.tolist(), T.rec.tolist()):
        w0, w1 = r[0] | r[1] << 32, r[2] | r[3] << 32
        out[s] = dict(type=w0 >> 62, prev=(w0 >> PBITS) & (IDS - 1), lo=w0 & ((1 << PBITS) - 1), kk=w1 & 0xFFFF, c=(w1 >> 16) & 7,
                      off=(r[2] ^ 0x80000000) - 0x80000000, dl=r[4], child=r[5], mask=sum(x << (32 * i) for i, x in enumerate(r[6:14])), head=r[14])
    return out


# ---- the index of the k_events cases: planes and run slots side by side in every group, at most 5 groups ---------------------------

@functools.lru_cache(maxsize=None)
def index_plain(n=None):
    rng = np.random.default_rng(20261021)
    p = []
    for g in range(5):
        p.append(rng.integers(0, 6, size=8 * lm.WIN, dtype=np.uint8))                      # 8 plane slots
        p.append(lm._runs_block(rng, 8 * lm.WIN, 30, None, syms=(0, 1, 2, 3, 4, 5)))      # a run slot of 8 windows
        p.append(lm._blocks(rng, 4, 2, 40, syms=(0, 1, 2, 3, 4, 5)))                       # four run slots of 2 windows
        p.append(rng.integers(0, 6, size=8 * lm.WIN, dtype=np.uint8))                      # planes up to the group border
    full = np.concatenate(p)
    out = full if n is None else full[:n].copy()
    out.setflags(write=False)
    return out


def slot_of(plain):
    """per window: (number of its slot, windows of that slot)"""
    masks = lm.slot_masks(plain)
    nwin = lm.n_windows(np.asarray(plain).size)
    start = ((masks[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)[:nwin]
    sid = np.cumsum(start) - 1
    return sid, np.bincount(sid)


def ev_facts(case):
    """per ("ix", lo, c) event of a case: lo, kk, c, n, the slots of lo, of lo + kk - 1 and of lo + kk with their kinds ('p' plane, 'r' run)"""
    plain = np.asarray(case.plain)
    sid, size = slot_of(plain)
    kind = lambda pos: "r" if size[sid[pos >> lm.WIN_BITS]] > 1 else "p"
    out = []
    for w in case.walkers:
        kk = w.K
        for e in w.events:
            lo, c = int(e[1]), int(e[2])
            hi = lo + kk
            out.append(dict(lo=lo, kk=kk, c=c, n=plain.size, s0=int(sid[lo >> 8]), s1=int(sid[(hi - 1) >> 8]), s2=int(sid[hi >> 8]), k0=kind(lo), k1=kind(hi - 1),
                            g0=lo >> 13, g1=(hi - 1) >> 13, off0=lo - (int(np.flatnonzero(sid == sid[lo >> 8])[0]) << 8),
                            end2=(hi & 255) == 0 and sid[hi >> 8] != sid[(hi - 1) >> 8]))
            kk -= int((plain[lo:hi] != c).sum())
    return out


def _ix_case(name, lo, kk, c, tags, n=None, d0=None, q=1):
    plain = index_plain(n)
    kept = int((plain[lo:lo + kk] == c).sum())
    assert 1 <= kept < kk, (name, kept, kk)
    return Case(name, [W(kk, kk // 2 + 1 if d0 is None else d0, events=[("ix", lo, c)], dels=(0,))], tags + ["k_events"], q=q, plain=plain)


def _find(plain, kk, c, ok, start=0):
    """the first lo >= start with ok(lo) whose interval of kk rows keeps some rows and drops some at symbol c"""
    for lo in range(start, plain.size - kk + 1):
        if ok(lo) and 1 <= int((plain[lo:lo + kk] == c).sum()) < kk:
            return lo
    raise AssertionError("no such interval")


def _ix_cases():
    P = index_plain()
    sid, size = slot_of(P)
    W8 = lm.WIN
    kind = lambda pos: "r" if size[sid[pos >> 8]] > 1 else "p"
    one = lambda lo, kk: sid[lo >> 8] == sid[(lo + kk) >> 8]
    out = []
    sym = lambda lo, kk: int(np.bincount(P[lo:lo + kk], minlength=6).argmax())
    def add(name, kk, ok, tags, c=None, start=0, q=1):
        if c is None:
            for cc in range(6):
                try:
                    lo = _find(P, kk, cc, ok, start)
                    break
                except AssertionError:
                    continue
            else:
                raise AssertionError(name)
        else:
            lo, cc = _find(P, kk, c, ok, start), c
        out.append(_ix_case(name, lo, kk, cc, tags, q=q))
    add("ev_inside_one_plane", 40, lambda lo: one(lo, 40) and kind(lo) == "p" and lo & 255 > 3, ["ev_one_plane"])
    add("ev_inside_one_run_slot", 40, lambda lo: one(lo, 40) and kind(lo) == "r" and lo & 255 > 3, ["ev_one_run"])
    for a, b in ("pp", "rr", "pr", "rp"):
        add("ev_across_%s%s" % (a, b), 60, lambda lo, a=a, b=b: sid[(lo + 59) >> 8] == sid[lo >> 8] + 1 and kind(lo) == a and kind(lo + 59) == b and (lo >> 13) == ((lo + 60) >> 13), ["ev_across_" + a + b])
    add("ev_across_group_border", 100, lambda lo: (lo >> 13) + 1 == (lo + 99) >> 13 and lo >> 13 == 1, ["ev_group_border"])
    add("ev_lo_at_slot_start", 33, lambda lo: lo & 255 == 0 and lo > 0 and sid[lo >> 8] != sid[(lo - 1) >> 8], ["ev_off0", "kk33"])
    add("ev_ends_at_slot_end", 32, lambda lo: (lo + 32) & 255 == 0 and sid[(lo + 32) >> 8] != sid[(lo + 31) >> 8], ["ev_end_at_slot_end", "kk32"])
    add("ev_kk2", 2, lambda lo: lo > 5000, ["kk2"])
    add("ev_kk255", 255, lambda lo: kind(lo) == "r" and lo > 9000, ["kk255"])
    add("ev_symbol0", 50, lambda lo: lo > 300, ["sym0"], c=0)
    add("ev_symbol5", 50, lambda lo: lo > 300, ["sym5"], c=5)
    for q, kk in ((2, 256), (2, 257), (2, 511), (4, 1023), (8, 2047)):
        add("ev_wide_q%d_kk%d" % (q, kk), kk, lambda lo, kk=kk: kind(lo) == "p" and lo > 700, ["kkwide%d" % kk], q=q)
    add("ev_wide_q8_over_many_slots", 2047, lambda lo: kind(lo) == "p" and kind(lo + 2046) == "p" and lo > 8192 + 100 and (lo >> 13) != ((lo + 2046) >> 13), ["ev_wide_many_slots"], q=8)
    # lo + kk == n, n on / below / above multiples of 256 and of 8192
    for n in (2 * lm.GRP, 2 * lm.GRP - 1, 2 * lm.GRP + 1, lm.GRP + 7 * W8, lm.GRP + 7 * W8 - 1, lm.GRP + 7 * W8 + 1):
        Pn = index_plain(n)
        for c in range(6):
            kept = int((Pn[n - 45:] == c).sum())
            if 1 <= kept < 45:
                out.append(_ix_case("ev_ends_at_n_%d" % n, n - 45, 45, c, ["ev_end_n_%s" % ("on" if n % 256 == 0 else "below" if n % 256 == 255 else "above") + ("8192" if abs(n - 2 * lm.GRP) <= 1 else "256")], n=n))
                break
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------------------

def _drop_seq(K, order):
    """events that drop the rows `order` (original indices) one at a time, as survivor indices"""
    surv, ev = list(range(K)), []
    for r in order:
        ev.append([surv.index(r)])
        surv.remove(r)
    return ev


def _chain(rng, n, kmax=40, craft=False, base=0):
    """n walkers, each linking out of its last stretch into the first stretch of the next; the first one settled by an exact walker
    (base: the place of the first one in the case's list of walkers)"""
    ws, dl = [], None
    for i in range(n):
        if craft and i >= 70 and i % 6 == 0:      # k_wj_round, `sidx >= zeros`: two walkers back almost every row dropped ...
            K, d0 = 250, 240
            ev = [list(range(205))]               # ... 45 survive, 35 of them below the suffix
        elif craft and i >= 70 and i % 6 == 1:    # ... and this one, reached with a negative offset, drops a row far above its unknown
            K, d0 = 120, dl - 10
            ev = [[100]]
        elif craft and i >= 70 and i % 6 == 3:    # `sidx < 0`: an interval that begins 5 rows below the one it is reached from and drops two of those
            K, d0 = 60, dl + 5
            ev = [[0, 3]]
        else:
            K = int(rng.integers(1, kmax + 1))
            d0 = int(rng.integers(0, K + 1))
            ev, s = [], K
            for _ in range(int(rng.integers(0, 3)) if K > 2 else 0):
                if s < 2:
                    break
                k = int(rng.integers(1, min(3, s - 1) + 1))
                ev.append(sorted(rng.choice(s, size=k, replace=False).tolist()))
                s -= k
        ws.append(W(K, d0, events=ev, dels=(0,) if i == 0 else ()))
        if i > 0:
            ws[i - 1].link = (base + i, 0, d0 - dl)
        surv = list(range(K))
        for e in ev:
            surv = [r for j, r in enumerate(surv) if j not in set(e)]
        dl = sum(1 for r in surv if r < d0)
    return ws


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261021)
    C = []
    # -- unknowns and widths at the word borders of the masks: one walker settled by an exact one, three events around the unknown
    for K in (1, 2, 31, 32, 33, 63, 64, 224, 254, 255):
        for d0 in sorted({0, 1, 31, 32, 33, 63, 64, 224, 254, 255, K} & set(range(K + 1))):
            ev = []
            if K > 3:
                s = list(range(K))
                picks = [[x for x in {d0 - 1, 0} if 0 <= x < K - 1], [x for x in {min(d0, K - 2)} if x >= 0]]
                for orig in picks:
                    orig = [r for r in orig if r in s][:len(s) - 1]
                    if orig:
                        ev.append(sorted(s.index(r) for r in orig))
                        s = [r for r in s if r not in orig]
            C.append(Case("K%d_d%d" % (K, d0), [W(K, d0, events=ev, dels=(0,))], ["K%d" % K] + ["d%d" % d0] * (d0 != 2)))
    for q, top in ((2, 511), (4, 1023), (8, 2047)):
        for K, d0 in ((256, 256), (257, 256), (257, 257), (top, 257), (top, top), (top, top - 1)):
            C.append(Case("wide_q%d_K%d_d%d" % (q, K, d0), [W(K, d0, events=[[0, 255, 256 if K > 257 else 255][:2 if K < 258 else 3], [d0 - 3] if d0 - 3 < K - 4 else [0]], dels=(0,))],
                          ["wideK%d" % K] * (K < 258) + ["wided%d" % d0] * (d0 < 258) + ["q%d" % q] * (K == d0 == top) + ["wide_bit255"], q=q))
    # -- which rows drop
    for b in (0, 31, 32, 254):
        C.append(Case("drop_bit%d" % b, [W(255, 255, events=[[b]], dels=(0,))], ["bit%d" % b, "one_dropped"]))
    C.append(Case("drop_all_but_one", [W(255, 200, events=[[i for i in range(255) if i != 199]], dels=(0,))], ["all_but_one"]))
    C.append(Case("drop_all_but_one_above", [W(255, 200, events=[[i for i in range(255) if i != 200]], dels=(0,))], ["all_but_one"]))
    shuf = rng.permutation(255).tolist()
    for nm, order in (("ascending", list(range(254))), ("descending", list(range(254, 0, -1))), ("shuffled", shuf[:254])):
        C.append(Case("one_at_a_time_" + nm, [W(255, 128, events=_drop_seq(255, order), dels=(0,))], ["peel_" + nm]))
    # -- event chains around the block of 8 ids; a second walker between the blocks; a jump to a far chunk
    for ne in (7, 8, 9, 15, 16, 17):
        C.append(Case("chain_%d_events" % ne, [W(100, 50, events=_drop_seq(100, list(range(40, 40 + ne))), dels=(0,)), W(9, 4, events=[[1], [2]], dels=(0,))], ["ev%d" % ne]))
    C.append(Case("chain_adjacent_blocks", [W(100, 50, events=_drop_seq(100, list(range(60, 30, -1))), dels=(0,))], ["adjacent_block"]))
    C.append(Case("chain_far_chunk", [W(100, 50, events=_drop_seq(100, list(range(45, 65))), dels=(0,), far=300), W(5, 2, events=[[4]], dels=(0,))], ["far_chunk"]))
    # -- links
    C.append(Case("link_from_first_offset0", [W(10, 4, dels=(0,), link=(1, 0, 0)), W(12, 4, events=[[1], [7]])], ["link_from_first", "off0"]))
    C.append(Case("link_from_first_offset_pos", [W(10, 4, dels=(0,), link=(1, 0, 3)), W(12, 7, events=[[1], [7]])], ["link_from_first", "off_pos"]))
    C.append(Case("link_from_last_offset_neg", [W(10, 6, events=[[0, 1], [5]], dels=(0,), link=(1, 0, -2)), W(12, 2, events=[[1], [7]])], ["link_from_last", "off_neg"]))
    C.append(Case("link_result_0", [W(10, 3, events=[[0, 1]], dels=(0,), link=(1, 0, -1)), W(12, 0, events=[[1]])], ["link_to_0"]))
    C.append(Case("link_result_K", [W(10, 3, events=[[0, 1]], dels=(0,), link=(1, 0, 11)), W(12, 12, events=[[1]])], ["link_to_K"]))
    C.append(Case("link_into_single", [W(10, 3, events=[[0, 1]], dels=(0,), link=(1, 0, 0)), W(1, 1)], ["link_into_single"]))
    C.append(Case("link_out_of_single", [W(1, 1, dels=(0,), link=(1, 0, 4)), W(9, 5, events=[[0], [0]], link=(2, 0, -3)), W(1, 0)], ["link_out_of_single", "link_into_single"]))
    # -- dependency paths
    for n in (1, 2, 3, 64, 65, 66, 67, 127, 128, 129):
        C.append(Case("path_%d" % n, _chain(rng, n), ["path%d" % n]))
    C.append(Case("path_1000", _chain(rng, 1000, kmax=12), ["path1000"]))
    C.append(Case("path_150_compositions", _chain(rng, 150, craft=True), ["wj_sidx_neg", "wj_sidx_above"]))
    # -- settled twice: the first stretch and a later one
    C.append(Case("del_first_and_later", [W(50, 20, events=[[3], [30], [10]], dels=(0, 2), link=(1, 0, 1)), W(30, 19, events=[[0]])], ["del_twice"]))
    # -- only a later stretch settled (a follower that never saw the first one), the first unknown pinned: no row dropped just below the d_t-th survivor
    C.append(Case("later_del_pinned", [W(50, 20, events=[[3], [30], [10]], dels=(2,), link=(1, 0, 1)), W(30, 19, events=[[0]])], ["later_del_pinned"],
                  must_v1=[(0, 2), (0, 3), (1, 0), (1, 1)]))
    C.append(Case("later_del_all_survivors_below_pinned", [W(20, 20, events=[[3], [5]], dels=(1,))], ["later_del_dt_is_width_pinned"], must_v1=[(0, 1), (0, 2)]))
    # ---- racy: states only late visibility produces ----
    C.append(Case("later_del_range", [W(50, 20, events=[[3], [19], [10]], dels=(2,), link=(1, 0, 1)), W(30, 19, events=[[0]])], ["later_del_range"], kind="racy",
                  must=[(0, 2), (0, 3), (1, 0), (1, 1)]))
    # ... and d_t = the number of survivors: the end of the interval stands in for the d_t-th survivor
    C.append(Case("later_del_all_survivors_below_range", [W(20, 18, events=[[3], [17, 18], [0]], dels=(2,))], ["later_del_dt_is_width_range"], kind="racy", must=[(0, 2), (0, 3)]))
    # a LINK written into an event stretch: the event is gone, the masks behind it stay per event (k_cum stops there)
    B = lambda dels, link=None: W(40, 30, events=[[2], [5], [0, 1, 20], [3, 9]], dels=dels, link=link)
    C.append(Case("link_over_event_first_settled", [W(10, 6, events=[[0]], dels=(0,), link=(1, 2, 23)), B((0,))], ["link_over_event", "stale_masks"], kind="racy",
                  must=[(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]))
    C.append(Case("link_over_event_first_unsettled", [W(10, 6, events=[[0]], dels=(0,), link=(1, 2, 23)), B(())], ["link_over_event"], kind="racy",
                  must=[(0, 0), (0, 1), (1, 2)]))
    # ... and that walker itself links out of its last stretch, which k_cum never reached, while a long path elsewhere starts the second chance: k_wj_init
    # must not take the last stretch's per-event mask for the cumulative one (the walker it ran into stays unsettled; k_resolve, hop by hop, settles it)
    C.append(Case("link_over_event_then_second_chance", [W(10, 6, events=[[0]], dels=(0,), link=(1, 2, 23)), B((0,), (2, 0, 0)), W(30, 23, events=[[1]])] + _chain(rng, 70, base=3),
                  ["link_over_event", "wj_unreached_mask"], kind="racy", must=[(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)] + [(k, None) for k in range(3, 73)]))
    C.append(Case("two_followers_one_stretch", [W(10, 6, dels=(0,), link=(2, 0, 2, "lost")), W(8, 3, events=[[0]], dels=(0,), link=(2, 0, 6)), W(20, 8, events=[[4]])],
                  ["link_lost"], kind="racy", must=[(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)]))
    C.append(Case("two_followers_the_loser_knew", [W(10, 6, dels=(0,), link=(2, 0, 2, "lost")), W(8, 3, events=[[0]], link=(2, 0, 6)), W(20, 8, events=[[4]])],
                  ["link_lost"], kind="racy", must=[(0, 0)]))
    C.extend(_ix_cases())
    names = [c.name for c in C]
    assert len(set(names)) == len(names)
    racy = sum(c.kind == "racy" for c in C)
    assert 3 * racy <= len(C), "at most a third of the cases may be racy"
    return C


def _any_walker(p):
    return lambda T, c: any(p(w, T, wi) for wi, w in enumerate(c.walkers))


def _evf(p):
    return lambda T, c: c.plain is not None and any(p(f) for f in ev_facts(c))


def _wj(kind):
    def pred(T, c):
        ws = c.walkers
        for k in range(RESW_MAXHOPS + 4, len(ws)):     # nodes k, k - 1 both beyond what k_resolve_w settled: round 1 composes them
            zeros = 256 - bin(T.cum[k - 2][-1]).count("1")
            off = ws[k - 2].link[2]
            for i in range(ws[k - 1].K):
                if T.cum[k - 1][-1] >> i & 1 and (i - off < 0 if kind == "neg" else i - off >= zeros):
                    return True
        return False
    return pred


BORDERS = {}
for _v in (1, 2, 31, 32, 33, 63, 64, 224, 254, 255):
    BORDERS["K%d" % _v] = (lambda v: lambda T, c: c.kind == "complete" and c.walkers[0].K == v)(_v)
for _v in (0, 1, 31, 32, 33, 63, 64, 224, 254, 255):
    BORDERS["d%d" % _v] = (lambda v: lambda T, c: c.kind == "complete" and c.walkers[0].d0 == v)(_v)
for _q in (2, 4, 8):
    BORDERS["q%d" % _q] = (lambda q: lambda T, c: c.q == q and any(w.K == 256 * q - 1 and w.d0 == 256 * q - 1 for w in c.walkers))(_q)
BORDERS.update({
    "wideK256": lambda T, c: c.q > 1 and c.walkers[0].K == 256, "wideK257": lambda T, c: c.q > 1 and c.walkers[0].K == 257,
    "wided256": lambda T, c: c.q > 1 and c.walkers[0].d0 == 256, "wided257": lambda T, c: c.q > 1 and c.walkers[0].d0 == 257,
    "wide_bit255": lambda T, c: c.q > 1 and any(m >> 255 & 1 for m in T.evmask[0]),
    "one_dropped": lambda T, c: any(bin(m).count("1") == 1 for m in T.evmask[0][1:]),
    "all_but_one": lambda T, c: any(len(s) == 1 for s in T.surv[0]) and len(c.walkers[0].events) == 1,
    "adjacent_block": lambda T, c: len(c.walkers) == 1 and T.sid[(0, 8)] == T.sid[(0, 7)] + 1,
    "far_chunk": lambda T, c: T.sid[(0, 16)] - T.sid[(0, 15)] > 2000 and not any(T.sid[(0, 15)] < s < T.sid[(0, 16)] for s in T.ids.tolist()),     # zero ids in between
    "link_from_first": lambda T, c: c.walkers[0].link is not None and not c.walkers[0].events,
    "link_from_last": lambda T, c: c.walkers[0].link is not None and len(c.walkers[0].events) > 0 and c.walkers[0].link[1] == 0,
    "off0": lambda T, c: c.walkers[0].link[2] == 0, "off_pos": lambda T, c: c.walkers[0].link[2] > 0, "off_neg": lambda T, c: c.walkers[0].link[2] < 0,
    "link_to_0": lambda T, c: c.kind == "complete" and c.walkers[1].d0 == 0 and c.walkers[0].link[:2] == (1, 0),
    "link_to_K": lambda T, c: c.kind == "complete" and c.walkers[1].d0 == c.walkers[1].K and c.walkers[0].link[:2] == (1, 0),
    "link_into_single": _any_walker(lambda w, T, wi: w.link is not None and T.sid[(w.link[0], w.link[1])] >= HALF),
    "link_out_of_single": _any_walker(lambda w, T, wi: w.link is not None and w.K == 1),
    "wj_sidx_neg": _wj("neg"), "wj_sidx_above": _wj("above"),
    "del_twice": lambda T, c: c.kind == "complete" and any(0 in w.dels and len(w.dels) > 1 for w in c.walkers),
    "later_del_pinned": lambda T, c: c.kind == "complete" and _later_del(T, c) == ("pinned", False),
    "later_del_range": lambda T, c: c.kind == "racy" and _later_del(T, c) == ("range", False),
    "later_del_dt_is_width_pinned": lambda T, c: c.kind == "complete" and _later_del(T, c) == ("pinned", True),
    "later_del_dt_is_width_range": lambda T, c: c.kind == "racy" and _later_del(T, c) == ("range", True),
    "link_over_event": lambda T, c: c.kind == "racy" and len(T.overwritten) == 1,
    "stale_masks": lambda T, c: c.kind == "racy" and len(T.overwritten) == 1 and 0 in c.walkers[1].dels and
        any(T.evmask[1][t] != T.cum[1][t] for t in range(c.walkers[0].link[1] + 1, len(T.d[1]))),
    "wj_unreached_mask": lambda T, c: c.kind == "racy" and len(T.overwritten) == 1 and c.walkers[1].link is not None and T.last[1] not in T.reached and
        T.evmask[1][-1] != T.cum[1][-1] and 0 in c.walkers[1].dels and second_chance(T, RESW_MAXHOPS),
    "link_lost": lambda T, c: c.kind == "racy" and sum(1 for w in c.walkers if w.link and len(w.link) > 3) == 1,
    "ev_one_plane": _evf(lambda f: f["s0"] == f["s2"] and f["k0"] == "p"), "ev_one_run": _evf(lambda f: f["s0"] == f["s2"] and f["k0"] == "r"),
    "ev_group_border": _evf(lambda f: f["g1"] == f["g0"] + 1),
    "ev_off0": _evf(lambda f: f["off0"] == 0), "ev_end_at_slot_end": _evf(lambda f: f["end2"] and f["s1"] == f["s0"]),
    "kk2": _evf(lambda f: f["kk"] == 2), "kk32": _evf(lambda f: f["kk"] == 32), "kk33": _evf(lambda f: f["kk"] == 33), "kk255": _evf(lambda f: f["kk"] == 255),
    "sym0": _evf(lambda f: f["c"] == 0), "sym5": _evf(lambda f: f["c"] == 5),
    "ev_wide_many_slots": _evf(lambda f: f["kk"] == 2047 and f["s1"] - f["s0"] >= 8 and f["g1"] != f["g0"]),
})
for _ab in ("pp", "rr", "pr", "rp"):
    BORDERS["ev_across_" + _ab] = _evf((lambda a, b: lambda f: f["s1"] == f["s0"] + 1 and f["k0"] == a and f["k1"] == b and f["g0"] == f["g1"])(*_ab))
for _kk in (256, 257, 511, 1023, 2047):
    BORDERS["kkwide%d" % _kk] = _evf((lambda kk: lambda f: f["kk"] == kk)(_kk))
for _w, _m in (("on", 0), ("below", 255), ("above", 1)):
    BORDERS["ev_end_n_%s256" % _w] = _evf((lambda m: lambda f: f["lo"] + f["kk"] == f["n"] and f["n"] % 256 == m and f["n"] % 8192 not in (0, 1, 8191))(_m))
    BORDERS["ev_end_n_%s8192" % _w] = _evf((lambda m: lambda f: f["lo"] + f["kk"] == f["n"] and f["n"] % 8192 == (m if m < 2 else 8191))(_m))
for _b in (0, 31, 32, 254):
    BORDERS["bit%d" % _b] = (lambda b: lambda T, c: c.q == 1 and any(m >> b & 1 for m in T.evmask[0]))(_b)
for _n in (7, 8, 9, 15, 16, 17):
    BORDERS["ev%d" % _n] = (lambda n: lambda T, c: len(c.walkers[0].events) == n and len(c.walkers) > 1 and (n < 8 or T.sid[(0, 8)] > T.sid[(1, 0)]))(_n)
for _n in (1, 2, 3, 64, 65, 66, 67, 127, 128, 129, 1000):
    BORDERS["path%d" % _n] = (lambda n: lambda T, c: T.path == n == len(c.walkers) and second_chance(T, RESW_MAXHOPS) == (n > RESW_MAXHOPS + 1))(_n)
for _o in ("ascending", "descending", "shuffled"):
    BORDERS["peel_" + _o] = (lambda o: lambda T, c: len(c.walkers[0].events) == 254 and len(T.surv[0][-1]) == 1 and
                             {"ascending": lambda r: r == sorted(r), "descending": lambda r: r == sorted(r, reverse=True), "shuffled": lambda r: r != sorted(r) and r != sorted(r, reverse=True)}[o](
                                 [T.surv[0][t - 1][c.walkers[0].events[t - 1][0]] for t in range(1, 255)]))(_o)


def _later_del(T, c):
    """a walker settled on a later stretch t only: (is its first unknown pinned to one position or left a range, is d_t the number of survivors).
    The first unknown lies behind the (d_t - 1)-th survivor and not behind the d_t-th; where every survivor is below the new suffix the d_t-th
    "survivor" is the end of the interval -- the mask bits from K up are never set, which is how k_cum finds it."""
    w = c.walkers[0]
    if not w.dels or 0 in w.dels:
        return None
    t = min(w.dels)
    dt, surv = T.d[0][t], T.surv[0][t]
    pmax, pmin = (surv[dt] if dt < len(surv) else w.K), (surv[dt - 1] + 1 if dt > 0 else 0)
    assert pmin <= w.d0 <= pmax
    return ("pinned" if pmin == pmax else "range", dt == len(surv))
