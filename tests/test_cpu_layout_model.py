"""The host model of the slot partition (tests/layout_model.py) on cases whose answer is worked out by hand, and the edge-case
generator: every case has the slot shape its name asks for."""
import numpy as np
import pytest

from tests import layout_model as lm


def _alternating(nruns, length, syms=(1, 2)):
    """`length` symbols in `nruns` runs of (nearly) equal length, symbols alternating"""
    cuts = np.linspace(0, length, nruns + 1).astype(np.int64)
    return np.concatenate([np.full(cuts[i + 1] - cuts[i], syms[i % len(syms)], dtype=np.uint8) for i in range(nruns)])


def test_two_windows_of_48_runs_are_one_run_slot_and_of_49_two_planes():
    # 512 symbols: windows 0 and 1 hold the symbols, window 2 (position 512) is empty; a block of 4 windows does not fit the 3
    b48 = _alternating(48, 512)
    b49 = _alternating(49, 512)
    assert list(lm.slot_masks(b48)) == [0b101]
    assert lm.slot_count(b48) == 2
    assert list(lm.slot_masks(b49)) == [0b111]
    assert lm.slot_count(b49) == 3
    assert lm.expected_bytes_index(b48) == 72 + 2 * 128 and lm.expected_bytes_index(b49) == 72 + 3 * 128


def test_a_run_across_a_window_border_counts_once():
    # 24 runs in window 0, the last one of them (symbol 3) goes on for 10 symbols into window 1, then 24 more runs: 48 maximal runs
    w0 = np.concatenate([_alternating(23, 246), np.full(10, 3, dtype=np.uint8)])
    w1 = np.concatenate([np.full(10, 3, dtype=np.uint8), _alternating(24, 246)])
    b = np.concatenate([w0, w1])
    assert b.size == 512 and (np.count_nonzero(np.diff(b.astype(int))) + 1) == 48
    assert lm.slot_count(b) == 2
    # the same symbols with the shared run cut in two (symbol 4 from the border on): 49 runs, three slots
    c = b.copy()
    c[256:266] = 4
    assert (np.count_nonzero(np.diff(c.astype(int))) + 1) == 49
    assert lm.slot_count(c) == 3


def test_a_single_run_of_8192():
    b = np.full(8192, 2, dtype=np.uint8)
    # group 0: 32 windows, one run -> one run slot of 32 windows; group 1: the empty window of position 8192, one bit-plane slot
    assert list(lm.slot_masks(b)) == [1, 1]
    assert lm.slot_count(b) == 2
    assert lm.expected_bytes_index(b) == 2 * 72 + 2 * 128


def test_a_group_of_32_windows_in_one_slot_and_one_that_is_not():
    b = np.concatenate([_alternating(48, 8192, (1, 2, 3)), np.full(100, 4, dtype=np.uint8)])
    assert list(lm.slot_masks(b)) == [1, 1] and lm.slot_count(b) == 2
    # 49 runs: the group falls apart into two slots of 16 windows (24 or 25 runs each)
    c = np.concatenate([_alternating(49, 8192, (1, 2, 3)), np.full(100, 4, dtype=np.uint8)])
    assert list(lm.slot_masks(c)) == [1 | 1 << 16, 1] and lm.slot_count(c) == 3


@pytest.mark.parametrize("r,nvw,slots", [(1, 1, 1), (255, 1, 1), (256, 2, 1), (257, 2, 1)])
def test_last_group_of_a_few_symbols(r, nvw, slots):
    b = np.concatenate([_alternating(40, 8192), np.full(r, 5, dtype=np.uint8)])
    assert lm.n_groups(b.size) == 2 and lm.n_windows(b.size) - 32 == nvw
    m = lm.slot_masks(b)
    assert m[0] == 1 and bin(int(m[1])).count("1") == slots
    assert lm.slot_count(b) == 1 + slots


def test_last_group_of_two_dense_windows_is_two_planes():
    rng = np.random.default_rng(5)
    b = np.concatenate([np.full(8192, 1, dtype=np.uint8), rng.integers(0, 6, size=300, dtype=np.uint8)])
    assert list(lm.slot_masks(b)) == [1, 0b11]


def test_cum():
    b = np.array([0, 3, 3, 5, 1, 3], dtype=np.uint8)
    c = lm.cum(b)
    assert c.shape == (7, 6) and c.dtype == np.int64
    assert list(c[0]) == [0] * 6 and list(c[6]) == [1, 1, 0, 3, 0, 1] and list(c[3]) == [1, 0, 0, 2, 0, 0]


def _full_groups(plain):
    return lm.slot_masks(plain)[: plain.size // lm.GRP]


@pytest.mark.parametrize("name,plain", lm.edge_cases(), ids=[c[0] for c in lm.edge_cases()])
def test_edge_case_has_its_shape(name, plain):
    assert plain.dtype == np.uint8 and 0 < plain.size <= 400000 and plain.max() <= 5
    nwin, ns = lm.n_windows(plain.size), lm.slot_count(plain)
    if name.startswith("runslot_"):
        sz = int(name[len("runslot_"):-1])
        want = sum(1 << w for w in range(0, 32, sz))
        assert all(int(m) == want for m in _full_groups(plain))
        assert ns < nwin
    elif name == "runs48_2w_slot":
        assert all(int(m) == 0x55555555 for m in _full_groups(plain))
    elif name == "runs49_2w_planes":
        assert ns == nwin
    elif name == "dense_random_every_slot_a_plane":
        assert ns == nwin
    elif name == "planes_and_run_slots_in_one_group":
        ms = _full_groups(plain)
        assert all(int(m) & 0xFFFF == 0xFFFF and int(m) >> 16 != 0xFFFF for m in ms)   # planes, then run slots, in every group
    elif name == "runs_on_window_and_group_borders":
        ends = np.flatnonzero(np.diff(plain.astype(np.int64))) + 1
        assert np.count_nonzero(ends % lm.WIN == 0) >= 40 and np.count_nonzero(ends % lm.GRP == 0) >= 2
        assert np.diff(np.concatenate([[0], ends, [plain.size]])).max() > 3 * lm.GRP
        assert ns < nwin // 8
    elif name.startswith("long_runs_of_symbol_"):
        s = int(name[-1])
        assert np.count_nonzero(plain == s) > plain.size // 2 and ns < nwin
    elif name.startswith("total_"):
        g, r = (int(x) for x in name[len("total_8192x"):].split("_plus_"))
        assert plain.size == 8192 * g + r
        if g:
            assert 0 < ns < nwin   # run slots and planes side by side
    else:
        raise AssertionError("no shape check for " + name)
