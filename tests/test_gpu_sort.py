"""The GPU suffix sorter (rb3sort_bwt, rb3gpu_sort.hip) against its restatement (tests/sort_model.py, itself held to the definition and
the host sorter in tests/test_cpu_sort.py) on inputs that sit on the borders of k_s_wsort, of the depth rule and of the key width:
every output -- BWT, suffix array, text-order words, every entry of the sampled inverse suffix array, the round count -- exactly."""
import ctypes

import numpy as np
import pytest

from tests import sort_model as sm

pytestmark = pytest.mark.gpu

FX = sm.fixtures()


def _steps(n):
    return sorted({s for s in (0, 1, 7, 100, n - 1, n, n + 5) if s >= 0})


def _rounds(h):
    return h.stats()["n_sort_rounds"]


def _check_handle(h, name, steps=None):
    """every way into sort_text_impl on one handle: (BWT, suffix array, text-order words) as they came back"""
    text, m = FX[name], sm.model(name)
    for step in _steps(m.n) if steps is None else steps:
        r0 = _rounds(h)
        p, ck = h.bwt_from_text(text, step)
        try:
            got = h.dev_download(p, m.n)
        finally:
            h.dev_free(p)
        assert np.array_equal(got, m.bwt), (name, step)
        assert _rounds(h) - r0 == m.rounds, (name, step)
        if step:
            assert np.array_equal(ck, m.ckrow(step)), (name, step)
        else:
            assert ck is None
    r0 = _rounds(h)
    d_bwt, d_tw, d_sa = h.sort_text_sa(text)
    try:
        bwt = h.dev_download(d_bwt, m.n)
        tw = h.dev_download(d_tw, m.n * 8).view(np.uint64)
        sa = h.dev_download(d_sa, m.n * 4).view(np.uint32)
    finally:
        for d in (d_bwt, d_tw, d_sa):
            h.dev_free(d)
    assert _rounds(h) - r0 == m.rounds, name
    assert np.array_equal(bwt, m.bwt) and np.array_equal(sa, m.sa) and np.array_equal(tw, m.tw), name
    assert np.array_equal(sa[(tw >> np.uint64(3)).astype(np.int64)], np.arange(m.n, dtype=np.uint32)), name   # sa[isa[p]] == p
    return bwt, sa, tw


def _check_sorter(h, s, name, step):
    """rb3gpu_sorter_bwt: the BWT and the sampled inverse suffix array"""
    L, text, m = h._lib, FX[name], sm.model(name)
    ck = np.full((m.n + step - 1) // step, -1, dtype=np.int64)
    p = ctypes.c_void_p()
    assert L.rb3gpu_sorter_bwt(s, m.n, text.ctypes.data, ctypes.byref(p), step, ck.ctypes.data) == 0
    try:
        got = h.dev_download(p, m.n)
    finally:
        assert L.rb3gpu_sorter_release(s, p) == 0
    assert np.array_equal(got, m.bwt) and np.array_equal(ck, m.ckrow(step)), (name, step)
    return got, ck


@pytest.mark.parametrize("name", list(FX))
def test_sorter_outputs_equal_the_model(name):
    from ropebwt3_amd import Rb3Gpu
    h = Rb3Gpu(verbose=1)
    try:
        _check_handle(h, name)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["family_129", "copies_127", "mix", "homopolymer_4097"])
def test_sorter_object_equals_the_model(name):
    from ropebwt3_amd import Rb3Gpu
    h = Rb3Gpu(verbose=1)
    s = h._lib.rb3gpu_sorter_create(0)
    assert s
    try:
        for step in (1, 7, 100, FX[name].size + 5):
            _check_sorter(h, s, name, step)
    finally:
        h._lib.rb3gpu_sorter_destroy(s)
        h.close()


def test_workspace_reuse_large_tiny_large():
    """one handle and one sorter object: the scratch of a large text is reused by a tiny one (the counters sit behind the flag bytes, at
    an offset that depends on n) and by the large one again -- every answer right, the first and the last the same"""
    from ropebwt3_amd import Rb3Gpu
    h = Rb3Gpu(verbose=1)
    s = h._lib.rb3gpu_sorter_create(0)
    assert s
    try:
        seen = []
        for name in ("family_1000", "one_symbol", "homopolymer_4097", "singles", "family_1000"):
            seen.append(_check_handle(h, name, steps=(7,)) + _check_sorter(h, s, name, 7))
        assert all(np.array_equal(a, b) for a, b in zip(seen[0], seen[-1]))
    finally:
        h._lib.rb3gpu_sorter_destroy(s)
        h.close()


def test_lone_sentinel():
    """the text [0]: the host sorter refuses it (an empty string), the GPU sorter takes it.  Pinned to the definition: the one suffix is
    row 0 and the symbol before it is the sentinel itself, no round."""
    from ropebwt3_amd import Rb3Gpu
    text = np.zeros(1, dtype=np.uint8)
    assert sm.brute_sa(text).tolist() == [0]
    h = Rb3Gpu(verbose=1)
    try:
        r0 = _rounds(h)
        p, ck = h.bwt_from_text(text, 1)
        try:
            assert h.dev_download(p, 1).tolist() == [0]
        finally:
            h.dev_free(p)
        assert ck.tolist() == [0] and _rounds(h) == r0
    finally:
        h.close()


def test_refusals_are_errors_and_leave_the_sorter_usable():
    """a text without its last sentinel, a symbol 6, no text, a negative step: an error code from the handle and from the sorter object,
    no round counted, and the next good text is sorted as if nothing had happened"""
    from ropebwt3_amd import Rb3Gpu
    good = FX["singles"]
    no_end = np.array([1, 2, 0, 3, 4], dtype=np.uint8)
    sym6 = good.copy()
    sym6[4] = 6
    h = Rb3Gpu(verbose=1)
    L = h._lib
    s = L.rb3gpu_sorter_create(0)
    assert s
    d = h.dev_alloc(good.size + 16)
    ck = np.zeros(good.size, dtype=np.int64)
    try:
        for text, n, step in ((no_end, no_end.size, 1), (sym6, sym6.size, 1), (good, 0, 1), (good, good.size, -1)):
            r0, p = _rounds(h), ctypes.c_void_p()
            assert L.rb3gpu_bwt_from_text(h._h, n, text.ctypes.data, d, step, ck.ctypes.data) < 0, (n, step)
            assert L.rb3gpu_sorter_bwt(s, n, text.ctypes.data, ctypes.byref(p), step, ck.ctypes.data) < 0, (n, step)
            assert _rounds(h) == r0
            _check_handle(h, "singles", steps=(1,))
            _check_sorter(h, s, "singles", 1)
    finally:
        h.dev_free(d)
        L.rb3gpu_sorter_destroy(s)
        h.close()
