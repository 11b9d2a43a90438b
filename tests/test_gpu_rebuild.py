"""The merge's rebuild kernels at their tier, row and window borders.

rb3gpu_sh_finish inserts any non-decreasing list of insertion points and rebuilds through build_index, so with from_plain for the old
index every case of tests/rebuild_model.py decides exactly what k_reb_group (both table sizes), k_plane_group (plain and LISTED), the
window and group kernels and the placement behind them see.  Every case runs under every rebuild setting, then a fixed mixed insertion
runs on top of its result (the second rebuild reads the slots the first one wrote); after each the whole index is compared with the
numpy reference: the symbols, rank at EVERY position, the C array, the maximal runs and the size the partition rule gives.  Under the
reb_force 1 settings the hand-over counters must equal the model's count of groups per tier, case by case: a border that moved by one
shows there even where the symbol path would rebuild the group just as well.

The fused single-synchronisation path (k_scan_place behind k_pos_finalize_check_rows) runs the families of tests/test_gpu_layouts.py
with reb_force 1 and is held to the same counts, the model fed with the oracle's insertion points."""
import functools

import numpy as np
import pytest

from ropebwt3_amd import Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError
from tests import layout_model as lm
from tests import rebuild_model as rm
from tests import util

pytestmark = pytest.mark.gpu

LAYOUTS = {"abs1": {}, "abs0": {"abs_limit": 0}, "abs2": {"abs_table": 1}}
T1_ALWAYS = rm.GRP      # no batch puts more rows than this into a group on average
# name -> (tune keys, reb_t1_rows the model is asked with, or None where the run-space rebuild must not run, or "any")
SETTINGS = {
    "default": ({}, "any"),
    "reb_force": ({"reb_force": 1}, rm.T1_ROWS_PER_GROUP),
    "reb_force_medium_tier_only": ({"reb_force": 1, "reb_t1_rows": 0}, 0),
    "reb_force_small_tier_first": ({"reb_force": 1, "reb_t1_rows": T1_ALWAYS}, T1_ALWAYS),
    "reb_never": ({"reb_force": -1}, None),
    "plane_rebuild_off_reb_force": ({"plane_rebuild": 0, "reb_force": 1}, rm.T1_ROWS_PER_GROUP),
    "window_rebuild": ({"window_rebuild": 1}, None),
    "group_rebuild": ({"group_rebuild": 1}, None),
}
COMBOS = [(s, "abs1") for s in SETTINGS] + [(s, lay) for lay in ("abs0", "abs2") for s in ("default", "reb_force")]
COUNTERS = ("n_reb_groups", "n_reb_groups_tier2", "n_reb_groups_window")


def _handle(layout, tune):
    h = Rb3Gpu(verbose=1)
    for k, v in list(LAYOUTS[layout].items()) + list(tune.items()):
        h.tune(k, v)
    return h


@functools.lru_cache(maxsize=None)
def _reference(i):
    """per case and step: (old, ka, sym, merged, its runs, its index size, {reb_t1_rows: hand-over counts}); computed once, never changed"""
    name, old, ka, sym, _ = rm.cases()[i]
    steps = []
    for step in (1, 2):
        if step == 2:
            old = steps[0][3]
            ka, sym = rm.second_step(old.size)
        merged = rm.insert(old, ka, sym)
        merged.setflags(write=False)
        F = rm.group_facts(old, ka, sym)
        ho = {t: rm.hand_over(old, ka, sym, t1_rows=t, facts=F) for t in (rm.T1_ROWS_PER_GROUP, 0, T1_ALWAYS)}
        steps.append((old, ka, sym, merged, rm.runs_of(merged), lm.expected_bytes_index(merged), ho))
    return name, steps


def _check(h, want, runs, nbytes, what):
    n = want.size
    assert h.get_tot() == n, what
    got = h.export_plain()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want) if got.size == n else np.zeros(1, dtype=np.int64)
        raise AssertionError("%s: export_plain differs at %d of %d positions, first %d (group %d, offset %d): %s != %s" % (
            what, bad.size, n, bad[0], bad[0] >> 13, bad[0] & 8191, got[bad[0]:bad[0] + 8].tolist(), want[bad[0]:bad[0] + 8].tolist()))
    cm = lm.cum(want)
    rk = h.rank1a(np.arange(n + 1, dtype=np.int64))
    if not np.array_equal(rk, cm):
        bad = np.flatnonzero((rk != cm).any(axis=1))
        raise AssertionError("%s: rank1a differs at %d of %d positions, first k = %d: %s != %s" % (what, bad.size, n + 1, bad[0], rk[bad[0]].tolist(), cm[bad[0]].tolist()))
    acc = h.get_acc()
    assert acc[0] == 0 and np.array_equal(acc[1:], np.cumsum(cm[n])), what
    assert h.export_runs() == runs, what
    assert h.stats()["bytes_index"] == nbytes, (what, h.stats()["bytes_index"], nbytes)


def _finish(h, ka, sym, jlo=0, iv_start=0):
    """sh_finish of the rows behind `jlo` rows of another interval, insertion points counted from iv_start"""
    d_sym = h.dev_upload(np.concatenate([np.full(jlo, 7, dtype=np.uint8), sym]))
    d_ka = h.dev_upload(np.concatenate([np.full(jlo, -1, dtype=np.int64), ka + iv_start]))
    try:
        h.sh_finish(jlo, ka.size, d_sym, d_ka, iv_start, commit=True)
    finally:
        h.dev_free(d_sym), h.dev_free(d_ka)


@pytest.mark.parametrize("setting,layout", COMBOS)
def test_rebuild_cases(setting, layout):
    tune, t1 = SETTINGS[setting]
    h = _handle(layout, tune)
    checked = 0
    try:
        for i in range(len(rm.cases())):
            name, steps = _reference(i)
            jlo, iv_start = ((0, 0), (5, 1234567), (300, 1))[i % 3]
            for step, (old, ka, sym, merged, runs, nbytes, ho) in enumerate(steps, 1):
                what = "%s / step %d / %s / %s" % (name, step, setting, layout)
                if step == 1:
                    h.from_plain(old)
                before = h.stats()
                _finish(h, ka, sym, jlo, iv_start)
                after = h.stats()
                _check(h, merged, runs, nbytes, what)
                grew = tuple(after[k] - before[k] for k in COUNTERS)
                if t1 is None:
                    assert grew == (0, 0, 0), (what, grew)
                elif t1 != "any":
                    assert grew == ho[t1], "%s: groups (seen, handed on by the small tier, handed on to the symbol path) %s, the model says %s" % (what, grew, ho[t1])
                checked += 1
    finally:
        h.close()
    assert checked == 2 * len(rm.cases()) >= 200


@pytest.mark.parametrize("setting", ["default", "reb_force", "reb_never", "group_rebuild"])
def test_bad_insertion_points_are_refused(setting):
    """k_pos_check answers before any rebuild kernel runs: an error, and the index as it was"""
    name, old, ka, sym, _ = next(c for c in rm.cases() if c[0] == "tier_nB128_tie")
    n, m = old.size, ka.size
    down = ka.copy()
    down[m // 2] -= 1                                     # not monotone
    below = ka + 1000
    below[0] = 999                                        # below the interval's start (iv_start 1000)
    beyond = ka.copy()
    beyond[-1] = n + 1                                    # behind the last position
    allbeyond = np.full(m, n + 1, dtype=np.int64)
    h = _handle("abs1", SETTINGS[setting][0])
    try:
        h.from_plain(old)
        runs, nbytes = rm.runs_of(old), lm.expected_bytes_index(old)
        for what, k, iv in (("not monotone", down, 0), ("below iv_start", below - 1000, 1000), ("beyond the end", beyond, 0), ("all beyond the end", allbeyond, 0)):
            with pytest.raises(Rb3GpuError):
                _finish(h, k, sym, 3, iv)
            _check(h, old, runs, nbytes, "%s / %s" % (what, setting))
        _finish(h, ka, sym)                               # and the handle still works
        _check(h, rm.insert(old, ka, sym), rm.runs_of(rm.insert(old, ka, sym)), lm.expected_bytes_index(rm.insert(old, ka, sym)), "after the refusals / " + setting)
    finally:
        h.close()


# ---- the production path: merge_text_dev (k_pos_finalize_check_rows -> group kernels -> k_scan_place, one synchronisation) ----

@functools.lru_cache(maxsize=None)
def _family_counts(kind, t1_rows):
    """per round of the family: the merged BWT and the model's hand-over counts, from the oracle's insertion points"""
    from tests import test_gpu_layouts as tl
    orc = util.Oracle()
    out, cur = [], None
    for t, b, want in tl._family(kind):
        if cur is None:
            out.append((t, want, None))
        else:
            rb, _ = orc.mg_rank(cur, b)
            ka = (rb >> 6) - np.arange(b.size, dtype=np.int64)
            assert np.array_equal(rm.insert(cur, ka, b), want)
            out.append((t, want, rm.hand_over(cur, ka, b, t1_rows=t1_rows)))
        cur = want
    return out


@pytest.mark.parametrize("t1_rows", [rm.T1_ROWS_PER_GROUP, T1_ALWAYS])
@pytest.mark.parametrize("kind", ["copies", "repeats"])
def test_single_sync_merge_hands_on_what_the_model_says(kind, t1_rows):
    h = _handle("abs1", {"reb_force": 1, "reb_t1_rows": t1_rows})
    try:
        moved = np.zeros(3, dtype=np.int64)
        for i, (t, want, ho) in enumerate(_family_counts(kind, t1_rows)):
            before = h.stats()
            if i == 0:
                h.from_plain(want)
                continue
            d, dtw = h.sort_text(t)
            h.merge_text_dev(d, dtw, t.size, host.walkers_text(t, 192), commit=True)
            h.dev_free(d), h.dev_free(dtw)
            after = h.stats()
            assert after["n_fallbacks"] == 0 and np.array_equal(h.export_plain(), want), (kind, i)
            grew = tuple(after[k] - before[k] for k in COUNTERS)
            assert grew == ho, "%s round %d: groups (seen, handed on by the small tier, handed on to the symbol path) %s, the model says %s" % (kind, i, grew, ho)
            moved += grew
        assert moved[0] > moved[2] > 0 and (t1_rows != T1_ALWAYS or moved[1] >= moved[2]), moved
    finally:
        h.close()
