"""The model of the merge's settle phase (tests/settle_model.py) held to the CPU oracle, and its table of stretch tables held to the
borders it claims.

Oracle pin: interval walkers on a small family round, walked in Python by plain rank on B1 from [0, n1], open stretches and events
where k_chain does (an interval of at most 255 rows; 1 <= kn < hi - lo); the model, given only the first unknown and the events, must
give ka_oracle - lo at every row across every event, and its link rule must hold wherever one walker's interval meets a row another
walker recorded.  Table checks: every border has a case that is on it (nothing is skipped: a missing border fails), at most a third
of the cases are racy, and the encoder's records read back as the fields the kernels read."""
import numpy as np
import pytest

from tests import layout_model as lm
from tests import settle_model as sm
from tests import util

KMAX = 255
STEP = 96          # text distance between walkers
MIN_AGE = 16       # RB3_TENT_MIN_AGE: a walker records tentatively only once it is this many steps old


def _family():
    rng = np.random.default_rng(20261021)
    g0 = util.random_genome(rng, 1500)
    rel = [g0, util.mutate(rng, g0, 0.004), g0.copy(), util.mutate(rng, g0, 0.01)]
    new = [util.mutate(rng, rel[1], 0.004)]
    return util.make_text(rel), util.make_text(new)


def _walk(b1, b2, ka):
    """per string of the batch, the rows of its backward walk in order; then per walker (one every STEP rows of a walk) its track:
    [(row, lo, hi)] from [0, n1] until the interval is empty or the string ends"""
    cum1, cum2 = lm.cum(b1), lm.cum(b2)
    C1 = np.concatenate([[0], np.cumsum(np.bincount(b1, minlength=6))])
    C2 = np.concatenate([[0], np.cumsum(np.bincount(b2, minlength=6))])
    m2 = int((b2 == 0).sum())
    tracks = []
    for s in range(m2):
        rows, r = [], s
        while True:
            rows.append(r)
            c = int(b2[r])
            if c == 0:
                break
            r = int(C2[c] + cum2[r, c])
        for start in range(0, len(rows) - 1, STEP):
            lo, hi, tr = 0, b1.size, []
            for r in rows[start:start + 3 * STEP]:
                assert lo <= ka[r] <= hi         # the interval of the suffixes that start with what was read holds the insertion point
                tr.append((r, lo, hi))
                c = int(b2[r])
                if c == 0 or hi == lo:
                    break
                lo, hi = int(C1[c] + cum1[lo, c]), int(C1[c] + cum1[hi, c])
            tracks.append(tr)
    return tracks


def _stretches(b1, b2, tr):
    """the model walker of a track: (first index of the track that carries a tentative record, W, stretch of every such index)"""
    first = next((i for i, (r, lo, hi) in enumerate(tr) if i >= MIN_AGE and 1 <= hi - lo <= KMAX), None)
    if first is None:
        return None
    events, st, t = [], {}, 0
    for i in range(first, len(tr)):
        r, lo, hi = tr[i]
        if hi == lo:
            break                                # exact from here on: final records
        st[i] = t
        if i + 1 < len(tr):
            kn = tr[i + 1][2] - tr[i + 1][1]
            if 1 <= kn < hi - lo:                # what k_chain notes: lo, the width, the symbol
                events.append(("ix", lo, int(b2[r])))
                t += 1
    return first, events, st


def test_model_truth_is_the_oracles_insertion_point(oracle):
    t1, t2 = _family()
    b1, b2 = oracle.bwt(t1), oracle.bwt(t2)
    rb, _ = oracle.mg_rank(b1, b2)
    ka = (rb >> 6) - np.arange(b2.size)
    tracks = _walk(b1, b2, ka)
    models, n_events, n_rows, n_links = [], 0, 0, 0
    for tr in tracks:
        s = _stretches(b1, b2, tr)
        models.append(s)
        if s is None:
            continue
        first, events, st = s
        r0, lo0, hi0 = tr[first]
        T = sm.build(sm.Case("pin", [sm.W(hi0 - lo0, int(ka[r0]) - lo0, events=events, dels=(0,))], [], plain=b1))
        for i, t in st.items():
            r, lo, hi = tr[i]
            assert T.d[0][t] == ka[r] - lo and len(T.surv[0][t]) == hi - lo, (i, t)
            n_rows += 1
        n_events += len(events)
    # junctions: walker A walks on into the rows of the walker that started STEP rows further along the same string
    recorded = {}                                 # row -> (walker, stretch, lo) of its first recorder
    for k, (tr, s) in enumerate(zip(tracks, models)):
        if s is not None:
            for i, t in s[2].items():
                if i < STEP:                          # its own segment: beyond it the rows are the next walker's
                    recorded.setdefault(tr[i][0], (k, t, tr[i][1]))
    for k, (tr, s) in enumerate(zip(tracks, models)):
        if s is None:
            continue
        first, events, st = s
        for i in sorted(st):
            r, lo, hi = tr[i]
            if r in recorded and recorded[r][0] != k:
                kb_, tb, lob = recorded[r]
                fb, evb, stb = models[kb_]
                trb = tracks[kb_]
                A = sm.W(tr[first][2] - tr[first][1], int(ka[tr[first][0]]) - tr[first][1], events=events[:st[i]], dels=(0,), link=(1, tb, lo - lob))
                B = sm.W(trb[fb][2] - trb[fb][1], int(ka[trb[fb][0]]) - trb[fb][1], events=evb)
                sm.build(sm.Case("junction", [A, B], [], kind="racy", must=[(0, 0)], plain=b1))   # build() refuses a link that contradicts the truth
                n_links += 1
                break
    assert n_rows > 2000 and n_events > 20 and n_links > 10, (n_rows, n_events, n_links)


def test_every_border_has_a_case_that_is_on_it():
    claimed, wrong = {}, []
    for c in sm.cases():
        T = sm.build(c)
        assert T.ids.size <= 4096 and (c.plain is None or c.plain.size <= 5 * lm.GRP), c.name     # nothing workload-sized
        for tag in c.tags:
            if tag == "k_events":
                continue
            assert tag in sm.BORDERS, (c.name, tag)
            if sm.BORDERS[tag](T, c):
                claimed.setdefault(tag, []).append(c.name)
            else:
                wrong.append((c.name, tag))
    assert not wrong, "cases that are not on the border they name: %s" % wrong
    missing = sorted(set(sm.BORDERS) - set(claimed))
    assert not missing, "borders without a case: %s" % missing


def test_racy_cases_are_few_and_name_what_must_settle():
    C = sm.cases()
    racy = [c for c in C if c.kind == "racy"]
    assert racy and 3 * len(racy) <= len(C)
    for c in racy:
        T = sm.build(c)
        assert c.must and T.must <= set(T.truth)    # non-empty; whatever is not named may stay unsettled, never wrong
    assert all(c.must is None for c in C if c.kind == "complete")
    # k_resolve walks forward only: where only a later stretch was settled it owes the stretches from there on, not the ones before -- there and nowhere else
    for c in C:
        if c.must_v1 is not None:
            T = sm.build(c)
            assert c.kind == "complete" and all(t.startswith("later_del_") for t in c.tags) and c.tags, c.name
            t0 = min(c.walkers[0].dels)
            assert T.must_v1 < T.must and T.must - T.must_v1 == {T.sid[(0, t)] for t in range(t0)}, c.name


def test_records_read_back_as_their_fields():
    for c in sm.cases():
        T = sm.build(c)
        D = sm.decode(T)
        ids = set(T.ids.tolist())
        assert all(0 <= s < T.n_a or sm.HALF <= s < sm.HALF + T.n_b for s in ids), c.name
        for (wi, t), s in T.sid.items():
            f, w = D[s], c.walkers[wi]
            assert f["dl"] == (1 + T.d[wi][t] if t in w.dels else 0)
            if s in T.won:                          # a link, whatever the stretch was before
                a = T.won[s]
                assert (f["type"], f["prev"], f["off"]) == (sm.LINK, T.last[a], c.walkers[a].link[2]) and D[T.last[a]]["child"] == s + 1
            elif t > 0:
                lo, sym = T.evrec[wi][t]
                assert (f["type"], f["prev"], f["lo"], f["kk"], f["c"]) == (sm.EVENT, T.sid[(wi, t - 1)], lo, len(T.surv[wi][t - 1]), sym)
                assert f["mask"] == (T.evmask[wi][t] if c.q == 1 else 0)
            else:
                assert f["type"] == 0 and f["mask"] == 0
            assert f["head"] == (T.first[wi] + 1 if t > 0 else 0)
            if t + 1 < len(T.d[wi]):
                assert f["child"] == T.sid[(wi, t + 1)] + 1 and T.sid[(wi, t + 1)] > s
                assert T.sid[(wi, t + 1)] == s + 1 or T.sid[(wi, t + 1)] % sm.BLOCK == 0     # the next id, or the first of a new chunk
            if t == 0:
                assert s >= sm.HALF if w.K == 1 else s % sm.BLOCK == 0
        # the chunk counters give the extent k_tent_extent works out, which covers every id in use
        assert T.n_a <= T.n_a_fused < T.n_a + sm.NCTR * sm.CHUNK and T.n_a_fused == int(T.ctr.max()) * sm.NCTR * sm.CHUNK


def test_build_refuses_what_contradicts_the_truth():
    for bad in ([sm.W(10, 11)], [sm.W(10, 3, events=[list(range(10))])], [sm.W(1, 0, events=[[0]])], [sm.W(300, 3)],
                [sm.W(10, 4, dels=(0,), link=(1, 0, 1)), sm.W(12, 4)], [sm.W(10, 4, dels=(0,), link=(1, 3, 0)), sm.W(12, 4)],
                [sm.W(10, 4, dels=(0,), link=(2, 0, 0)), sm.W(10, 4, dels=(0,), link=(2, 0, 0)), sm.W(12, 4)]):
        with pytest.raises(AssertionError):
            sm.build(sm.Case("bad", bad, []))
    with pytest.raises(AssertionError):
        sm.build(sm.Case("bad", [sm.W(40, 3, events=[("ix", sm.index_plain().size - 10, 1)], dels=(0,))], [], plain=sm.index_plain()))
