"""The merge's settle kernels on hand-made stretch tables at their borders.

rb3gpu_test_settle (test build of the library) puts a table of tentative stretches on the device and runs the settle on it through the
host functions a merge calls, so every case of tests/settle_model.py decides exactly what k_events, k_cum, k_resolve_w, k_sfin, the
pointer-jumping k_wj_*, their wide-mask twins and k_resolve see.  Every case runs under every engine setting:
  soundness     sfin[s] is 0 or 1 + the true unknown, for every stretch of every case;
  completeness  every stretch of a `complete` case is settled, and the named stretches of a `racy` one;
  masks         k_events leaves the model's drop-out masks bit for bit, k_cum the union in first-interval coordinates;
  second chance it runs exactly where a dependency path is longer than maxhops + 1 walkers.
A real merge on the same handle afterwards shows that the seam keeps the handle's bookkeeping of the table."""
import functools

import numpy as np
import pytest

from ropebwt3_amd import Rb3Gpu, host
from tests import settle_model as sm
from tests import util

pytestmark = pytest.mark.gpu

# name -> (engine, maxhops, q the masks of q = 1 cases are zero-extended to, tune keys, chunk counters instead of n_a)
ONE_BLOCK = {"ev_blocks": 1, "cum_blocks": 1, "resw_blocks": 1, "sfin_blocks": 1}     # (a setting with tune keys gets handles of its own: nothing to restore)
SETTINGS = {
    "merge": (0, sm.RESW_MAXHOPS, 1, {}, False),
    "merge_every_hop": (0, sm.IDS, 1, {}, False),          # the staged path's call: no second chance
    "merge_fused_extent": (0, sm.RESW_MAXHOPS, 1, {}, True),
    "merge_one_block": (0, sm.RESW_MAXHOPS, 1, ONE_BLOCK, False),
    "resolve_v1": (1, sm.RESW_MAXHOPS, 1, {}, False),
    "wide_q2": (0, sm.RESW_MAXHOPS, 2, {}, False),
    "wide_q4": (0, sm.RESW_MAXHOPS, 4, {}, False),
    "wide_q8": (0, sm.RESW_MAXHOPS, 8, {}, False),
    "wide_q8_every_hop": (0, sm.IDS, 8, {}, False),
}


@functools.lru_cache(maxsize=None)
def _table(i):
    """built once per case, never changed"""
    T = sm.build(sm.cases()[i])
    for a in (T.ids, T.rec, T.ev):
        a.setflags(write=False)
    return T


class _Handles:
    """one handle per header layout; the index of the k_events cases is loaded when a case asks for another one"""

    def __init__(self, more=None):
        self.h, self.n = {}, {}
        for lay, tune in (("abs1", {}), ("abs0", {"abs_limit": 0})):
            h = Rb3Gpu(verbose=1, hooks=True)
            for k, v in list(tune.items()) + list((more or {}).items()):
                h.tune(k, v)
            self.h[lay], self.n[lay] = h, None

    def get(self, lay, plain):
        h = self.h[lay]
        if plain is not None and self.n[lay] != plain.size:
            h.from_plain(np.array(plain))
            self.n[lay] = plain.size
        elif plain is None and self.n[lay] is None:
            self.get(lay, sm.index_plain())
        return h

    def close(self):
        for h in self.h.values():
            h.close()


@pytest.fixture(scope="module")
def handles():
    H = _Handles()
    yield H
    H.close()


def _wide(a, q):
    out = np.zeros((a.shape[0], 8 * q), dtype=np.uint32)
    out[:, :a.shape[1]] = a
    return out


def _run_case(h, i, engine, maxhops, q, fused):
    """one case under one setting; returns the failures as strings"""
    case, T = sm.cases()[i], _table(i)
    if case.q > 1:
        if engine == 1 or q > 1 or fused:
            return []          # wide-only cases run at their own width
        q = case.q
    fails = []
    kw = dict(q=q, maxhops=maxhops, engine=engine, chunk_ctr=T.ctr if fused else None)
    n_a = T.n_a_fused if fused else T.n_a
    ev = _wide(T.ev, q)
    if case.plain is not None:
        rec = T.rec.copy()
        rec[:, 6:14] = 0       # k_events makes the masks itself, in both phases that run it
        r = h.test_settle(T.ids, rec, n_a, T.n_b, phase=0, masks=np.zeros_like(ev) if q > 1 else None, **kw)
        if not np.array_equal(r["masks"], ev):
            fails.append("%s: k_events masks differ at ids %s" % (case.name, T.ids[(r["masks"] != ev).any(axis=1)].tolist()[:6]))
        if r["sfin"].any():
            fails.append("%s: k_events alone settled something" % case.name)
        r = h.test_settle(T.ids, rec, n_a, T.n_b, phase=2, masks=np.zeros_like(ev) if q > 1 else None, **kw)
    else:
        r = h.test_settle(T.ids, T.rec, n_a, T.n_b, phase=1, masks=ev if q > 1 else None, **kw)
    try:
        sm.check(T, case, r["sfin"], engine)
    except AssertionError as e:
        fails.append(str(e))
    if engine == 0:
        want_sc = sm.second_chance(T, maxhops)
        if r["second_chance"] != want_sc or (r["bad"][2] != 0) != want_sc:
            fails.append("%s: second chance ran %s, bad[2] = %d, longest path %d walkers" % (case.name, r["second_chance"], int(r["bad"][2]), T.path))
        for s, m in T.reached.items():
            if r["masks"][T.row[s]].tolist() != sm.words(m, 8 * q):
                fails.append("%s: cumulative mask of stretch %d differs" % (case.name, s))
                break
    else:
        if not np.array_equal(r["masks"], ev):
            fails.append("%s: k_resolve changed the masks" % case.name)
    return fails


@pytest.mark.parametrize("layout", ["abs1", "abs0"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_settle_table(handles, setting, layout):
    engine, maxhops, q, tune, fused = SETTINGS[setting]
    fails = []
    own = _Handles(tune) if tune else None
    try:
        for i, case in enumerate(sm.cases()):
            if layout == "abs0" and case.plain is None:
                continue           # the header layout is k_events' business only
            fails += _run_case((own or handles).get(layout, case.plain), i, engine, maxhops, q, fused)
    finally:
        if own:
            own.close()
    assert not fails, "%d failures:\n%s" % (len(fails), "\n".join(fails[:40]))


def test_seam_refuses_a_malformed_table(handles):
    """nothing that would take a kernel outside the table or the index reaches the device"""
    from ropebwt3_amd.gpu import Rb3GpuError
    h = handles.get("abs1", None)
    i = [c.name for c in sm.cases()].index("chain_9_events")
    T = _table(i)
    for what, (col, val) in {"child beyond the extent": (5, T.n_a + 1), "head beyond the extent": (14, T.n_a + 9), "interval of one row": (2, 1), "prev in the gap": (1, (sm.EVENT << 30) | ((sm.HALF - 8) << 6))}.items():
        rec = T.rec.copy()
        rec[9 if col != 5 else 0, col] = val
        with pytest.raises(Rb3GpuError):
            h.test_settle(T.ids, rec, T.n_a, T.n_b)
    with pytest.raises(Rb3GpuError):
        h.test_settle(T.ids[::-1].copy(), T.rec, T.n_a, T.n_b)
    with pytest.raises(Rb3GpuError):
        h.test_settle(T.ids, T.rec, T.n_a - 8, T.n_b)
    j = [c.name for c in sm.cases()].index("ev_kk255")
    Tj = _table(j)
    rec = Tj.rec.copy()
    rec[1, 0] = sm.index_plain().size - 100      # lo + kk beyond the index
    with pytest.raises(Rb3GpuError):
        h.test_settle(Tj.ids, rec, Tj.n_a, Tj.n_b, phase=0)
    rel = Rb3Gpu(verbose=1)                      # the release library has no seam
    with pytest.raises(Rb3GpuError) as e:
        rel.test_settle(T.ids, T.rec, T.n_a, T.n_b)
    assert e.value.code == -7
    rel.close()


def test_a_merge_after_the_seam(handles, oracle):
    """a family round through merge_text_dev on a handle that has just served the seam: the part of the table the seam used is cleared"""
    h = handles.get("abs1", None)
    big = [c.name for c in sm.cases()].index("path_1000")
    T = _table(big)
    h.test_settle(T.ids, T.rec, T.n_a, T.n_b)
    rng = np.random.default_rng(9)
    g0 = util.random_genome(rng, 12000)
    rel = [g0, util.mutate(rng, g0, 0.002), util.mutate(rng, g0, 0.001), g0.copy()]
    b1 = host.build_bwt(util.make_text(rel))
    h.from_plain(b1)
    handles.n["abs1"] = None
    t2 = util.make_text([util.mutate(rng, rel[1], 0.001), rel[2].copy()])
    d_bwt, d_tw = h.sort_text(t2)
    before = h.stats()
    h.merge_text_dev(d_bwt, d_tw, t2.size, host.walkers_text(t2, 128), commit=True)
    h.dev_free(d_bwt)
    h.dev_free(d_tw)
    st = h.stats()
    assert st["n_fallbacks"] == before["n_fallbacks"]     # nothing of the seam's table was taken for a record of this merge
    assert np.array_equal(h.export_plain(), oracle.merge(b1, host.build_bwt(t2.copy())))
    r = h.test_settle(T.ids, T.rec, T.n_a, T.n_b)         # and the other way round
    sm.check(T, sm.cases()[big], r["sfin"])
