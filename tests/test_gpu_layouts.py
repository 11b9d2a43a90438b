"""Rank and kount on every slot writer and every slot-header layout, checked exhaustively.

Every answer of the engine goes through one decode (oct_rank_issue / oct_rank_finish) of the block array of rb3gpu_layout.h.  What it
reads depends on the writer that filled the slots and on the header layout of the index (IdxView.abs):
  1  the default below 2^32 symbols: slot headers hold the whole LF base
  0  headers counted from the group start (tune abs_limit 0)
  2  headers hold the low 32 bits of the LF base, the rest comes from the table of bases every 2^31 symbols (k_sb_table): the layout
     of 2^32 symbols and more, forced on a small index by tune abs_table 1
Here every writer (from_plain, from_runs, the device FMD decoder in one pass and in chunks of 1 and 3 groups, and the merge rebuilds
in each of their settings) runs in every layout on plain sequences made to hit one slot shape each (tests/layout_model.py), and
rank1a is compared with the plain cumulative counts at EVERY position; the index's size must be the one the partition rule gives.
kount runs in layouts 0 and 2 and over handles of mixed layouts against the k-mer model (tests/kount_model.py)."""
import functools
import os

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from tests import kount_model as km
from tests import layout_model as lm
from tests import util

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYOUTS = {"abs1": {}, "abs0": {"abs_limit": 0}, "abs2": {"abs_table": 1}}
REBUILDS = {"default": {}, "group_rebuild": {"group_rebuild": 1}, "window_rebuild": {"window_rebuild": 1},
            "plane_rebuild_off": {"plane_rebuild": 0}, "reb_force": {"reb_force": 1}}
CASES = dict(lm.edge_cases())


def _handle(layout, **tune):
    """a fresh handle, tuned before any index exists"""
    h = Rb3Gpu(verbose=1)
    for k, v in list(LAYOUTS[layout].items()) + list(tune.items()):
        h.tune(k, v)
    return h


def _check(h, plain, cm, what):
    n = plain.size
    assert h.get_tot() == n, what
    assert np.array_equal(h.export_plain(), plain), what
    got = h.rank1a(np.arange(n + 1, dtype=np.int64))
    if not np.array_equal(got, cm):
        bad = np.flatnonzero((got != cm).any(axis=1))
        raise AssertionError("%s: rank1a differs at %d of %d positions, first k = %d: %s != %s" % (what, bad.size, n + 1, bad[0], got[bad[0]].tolist(), cm[bad[0]].tolist()))
    acc = h.get_acc()
    assert acc[0] == 0 and np.array_equal(acc[1:], np.cumsum(cm[n])), what
    assert h.stats()["bytes_index"] == lm.expected_bytes_index(plain), (what, h.stats()["bytes_index"], lm.expected_bytes_index(plain))


@functools.lru_cache(maxsize=None)
def _golden(name):
    return km.golden_plain(GOLDEN, name + ".fmd", _build.BIN_CLI)


def _all_writers(plain, layout, tmp_path, name):
    """from_plain, from_runs(export_runs()), from_fmd_file with load_chunk 1 and 3, each in `layout`"""
    cm = lm.cum(plain)
    src = _handle("abs1")
    try:
        src.from_plain(plain)
        runs = src.export_runs()
        fn = str(tmp_path / ("%s.fmd" % name))
        with open(fn, "wb") as f:
            f.write(host.fmd_bytes_from_words(src.export_fmd_words(), src.get_acc()))
    finally:
        src.close()
    assert sum(l for _, l in runs) == plain.size
    assert np.array_equal(np.repeat(np.array([c for c, _ in runs], dtype=np.uint8), [l for _, l in runs]), plain)
    writers = [("from_plain", {}, lambda h: h.from_plain(plain)), ("from_runs", {}, lambda h: h.from_runs(runs)),
               ("fmd_chunk1", {"load_chunk": 1}, lambda h: h.from_fmd_file(fn)), ("fmd_chunk3", {"load_chunk": 3}, lambda h: h.from_fmd_file(fn))]
    for wname, tune, write in writers:
        h = _handle(layout, **tune)
        try:
            write(h)
            _check(h, plain, cm, "%s / %s / %s" % (name, wname, layout))
        finally:
            h.close()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_writers_on_edge_cases(name, layout, tmp_path):
    _all_writers(CASES[name], layout, tmp_path, name)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", ["longruns", "copies3000", "edge_chars", "genomes12"])
def test_writers_on_golden_indexes(name, layout, tmp_path):
    _all_writers(_golden(name), layout, tmp_path, name)


# ---- merge writers: a family of sequences with homopolymers, tandem repeats and exact copies, merged round by round ----

def _family_seq(rng, n, p_random):
    parts, tot = [], 0
    while tot < n:
        r = rng.random()
        if r < p_random:
            p = util.random_genome(rng, int(rng.integers(50, 400)))
        elif r < (1 + p_random) / 2:
            p = np.full(int(rng.integers(20, 300)), rng.integers(1, 5), dtype=np.uint8)                     # homopolymer
        else:
            p = np.tile(util.random_genome(rng, int(rng.integers(1, 7))), int(rng.integers(10, 80)))       # tandem repeat
        parts.append(p)
        tot += p.size
    return np.concatenate(parts)[:n]


@functools.lru_cache(maxsize=None)
def _family(kind="repeats"):
    """[(text of the round, its BWT, the merged plain BWT after the round)] for 8 rounds; the truth is the CPU oracle's merge.
    repeats: less than half of the windows are bit-plane slots from the first round on, so the default merge takes the run-space
    rebuild too.  copies: 12 to 19 near-identical copies of a random genome, an index of run slots of 2 and then 4 windows (and a
    handful of planes), with dozens of aligned 4-window blocks of exactly 48 runs from the fourth round on: the border of the
    partition rule"""
    orc = util.Oracle()
    if kind == "repeats":
        rng = np.random.default_rng(611)
        g0 = _family_seq(rng, 12000, 0.2)
        batches = [[g0, g0.copy(), util.mutate(rng, g0, 0.0005)], [g0.copy()], [util.mutate(rng, g0, 0.001)], [_family_seq(rng, 6000, 0.5), g0.copy()],
                   util.reads_from(rng, g0, 120, 150, err=0.005), [util.mutate(rng, g0, 0.0005), g0.copy()], [g0[:7000].copy(), _family_seq(rng, 3000, 0.2)], [g0.copy()]]
    else:
        rng = np.random.default_rng(612)
        g0 = util.random_genome(rng, 12000)
        batches = [[util.mutate(rng, g0, 0.0002) for _ in range(12)]] + [[util.mutate(rng, g0, 0.0003)] for _ in range(7)]
    out, cur = [], None
    for seqs in batches:
        t = util.make_text(seqs)
        b = host.build_bwt(t.copy())
        cur = b if cur is None else orc.merge(cur, b)
        out.append((t, b, cur))
    return out


def _merge_family(h, check=None, kind="repeats"):
    for i, (t, b, want) in enumerate(_family(kind)):
        if i == 0:
            h.from_plain(b)
        elif i % 2:
            h.merge_plain(b)   # LF walk over the batch BWT
        else:
            d, dtw = h.sort_text(t)
            h.merge_text_dev(d, dtw, t.size, host.walkers_text(t, 192), commit=True)
            h.dev_free(d), h.dev_free(dtw)
        if check:
            check(i, want)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("rebuild", sorted(REBUILDS))
@pytest.mark.parametrize("kind", ["repeats", "copies"])
def test_merge_rebuilds(kind, rebuild, layout):
    h = _handle(layout, **REBUILDS[rebuild])
    shapes = []

    def check(i, want):
        _check(h, want, lm.cum(want), "%s / %s / %s / round %d" % (kind, rebuild, layout, i))
        assert h.stats()["n_fallbacks"] == 0, (rebuild, layout, i)
        shapes.append((lm.slot_count(want), lm.n_windows(want.size)))
    try:
        _merge_family(h, check, kind)
        st = h.stats()
    finally:
        h.close()
    assert all(0 < ns < nw for ns, nw in shapes)   # run slots and bit planes side by side in every index
    # the setting took the rebuild it names: the run-space kernel (k_reb_group) or not
    if rebuild in ("reb_force", "default"):
        assert st["n_reb_groups"] > 0, st
    elif rebuild in ("group_rebuild", "window_rebuild"):
        assert st["n_reb_groups"] == 0, st


# ---- kount in layouts 0 and 2, and over handles of mixed layouts ----

KOUNT_KS = (1, 12, 31, 32, 33, 64, 65)   # the word borders of the 2-bit k-mer code


@functools.lru_cache(maxsize=None)
def _plain(name):
    return _family()[-1][2] if name == "family" else _golden(name)


@functools.lru_cache(maxsize=None)
def _strings(name):
    return km.strings_of(_plain(name))


@functools.lru_cache(maxsize=None)
def _model(name, k, m):
    if m >= 1 and m != 1:
        kk, cc = _model(name, k, 1)
        keep = cc[:, 0] >= m
        return kk[keep], cc[keep]
    return km.kount_strings([_strings(name)], k, m)


def _kount_handle(name, layout):
    h = _handle(layout)
    if name == "family":
        _merge_family(h)   # the index as the merge writers leave it in this layout
    else:
        h.from_plain(_plain(name))
    assert np.array_equal(h.export_plain(), _plain(name))
    return h


@pytest.mark.parametrize("layout", ["abs0", "abs2"])
@pytest.mark.parametrize("name", ["reads_fq", "longruns", "copies3000", "family"])
def test_kount_in_layout(name, layout):
    h, d = _kount_handle(name, layout), _kount_handle(name, "abs1")
    try:
        for k in KOUNT_KS:
            for m in ((0, 1, 2) if k == 1 else (1, 2)):
                got, ref = h.kount(k, m), d.kount(k, m)
                wk, wc = _model(name, k, m)
                assert got[0].shape == wk.shape and np.array_equal(got[0], wk) and np.array_equal(got[1], wc), (name, layout, k, m)
                assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), (name, layout, k, m)
    finally:
        h.close(), d.close()


@pytest.mark.parametrize("name,k,m,cap", [("copies3000", 31, 1, 4), ("family", 33, 2, 4), ("reads_fq", 31, 2, 1000), ("family", 12, 1, 1000)])
def test_kount_sliced_in_layout2(name, k, m, cap):
    h = _kount_handle(name, "abs2")
    try:
        st = {}
        kk, cc = h.kount(k, m, max_level_nodes=cap, stats=st)
        wk, wc = _model(name, k, m)
        assert np.array_equal(kk, wk) and np.array_equal(cc, wc)
        assert st["n_slices"] > 1 and st["n_out"] == wk.shape[0]
    finally:
        h.close()


@pytest.mark.parametrize("k", [12, 32, 33])
def test_kount_same_bwt_in_three_layouts(k):
    """one index in layouts 1, 0 and 2 walked together: every count column is the single-index model's column"""
    hs = [_kount_handle("reads_fq", lay) for lay in ("abs1", "abs0", "abs2")]
    try:
        for m in (1, 2):
            kk, cc = hs[0].kount(k, m, others=hs[1:])
            wk, wc = _model("reads_fq", k, m)
            assert cc.shape == (wk.shape[0], 3) and np.array_equal(kk, wk)
            for j in range(3):
                assert np.array_equal(cc[:, j], wc[:, 0]), (k, m, j)
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("k,m", [(12, 1), (31, 2), (64, 1)])
def test_kount_different_bwts_in_mixed_layouts(k, m):
    names, lays = ["copies3000", "family", "longruns"], ["abs1", "abs0", "abs2"]
    hs = [_kount_handle(n, lay) for n, lay in zip(names, lays)]
    try:
        kk, cc = hs[0].kount(k, m, others=hs[1:])
        wk, wc = km.kount_strings([_strings(n) for n in names], k, m)
        assert np.array_equal(kk, wk) and np.array_equal(cc, wc)
    finally:
        for h in hs:
            h.close()
