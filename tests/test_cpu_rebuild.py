"""The model of the merge's rebuild (tests/rebuild_model.py) held to the CPU oracle, and its table of insertions held to the borders
it claims: every border of the tier, ties and planes lists has a case on each side according to group_facts (nothing is skipped:
a missing border fails), every ties and geometry case can tell a reversed tie and a moved insertion point from the right answer,
and the model's slot partition is the one of layout_model."""
import numpy as np
import pytest

from tests import layout_model as lm
from tests import rebuild_model as rm
from tests import util


def _batches():
    rng = np.random.default_rng(77)
    g0 = util.random_genome(rng, 9000)
    family = [g0, util.mutate(rng, g0, 0.001)], [util.mutate(rng, g0, 0.002), g0.copy()]
    reads = [g0], util.reads_from(rng, g0, 150, 100, err=0.01)
    return {"family_round": family, "reads": reads}


@pytest.mark.parametrize("name", ["family_round", "reads"])
def test_insert_is_the_oracles_merge(name, oracle):
    first, second = _batches()[name]
    b1, b2 = oracle.bwt(util.make_text(first)), oracle.bwt(util.make_text(second))
    rb, _ = oracle.mg_rank(b1, b2)
    pos = rb >> 6
    ka = pos - np.arange(b2.size)
    assert (np.diff(ka) >= 0).all() and (np.diff(ka) == 0).any()     # real batches have ties
    assert np.array_equal(rm.insert(b1, ka, b2), oracle.merge(b1, b2))


def test_insert_keeps_ties_in_row_order():
    old = np.array([1, 1, 2], dtype=np.uint8)
    got = rm.insert(old, [0, 1, 1, 1, 3, 3], [5, 3, 4, 0, 2, 1])
    assert got.tolist() == [5, 1, 3, 4, 0, 1, 2, 2, 1]
    assert np.array_equal(got, np.insert(old, [0, 1, 1, 1, 3, 3], [5, 3, 4, 0, 2, 1]))
    assert rm.runs_of(got) == [(5, 1), (1, 1), (3, 1), (4, 1), (0, 1), (1, 1), (2, 2), (1, 1)]


def test_group_facts_on_a_hand_made_group():
    """one run of 3 x 8192 symbols; rows at three points of group 1: absorbed, a tie that starts absorbed and then differs, a differing row"""
    old = np.full(3 * rm.GRP + 10, 2, dtype=np.uint8)
    ka = np.array([9000, 9100, 9100, 9100, 9100, 9200], dtype=np.int64)
    sym = np.array([2, 2, 3, 2, 2, 4], dtype=np.uint8)
    F = rm.group_facts(old, ka, sym)
    assert [f["nb"] for f in F] == [0, 6, 0, 0] and [f["A0"] for f in F] == [0, 8192, 16378, 24570]
    f = F[1]
    assert (f["ns"], f["n_single"], f["nB"], f["nC"], f["new_slots"]) == (1, 0, 4, 2, 1)
    assert f["ties"] == [(0, 1, 808, -1, True), (1, 4, 908, 1, True), (5, 1, 1008, 0, True)]
    assert F[2]["ns"] == 2 and [rm.tier(x) for x in F] == [1, 1, 1, 3] and F[3]["last"]
    assert rm.hand_over(old, ka, sym) == (4, 1, 1)
    assert rm.hand_over(old, ka, sym, t1_rows=0) == (4, 0, 1)
    dense = np.random.default_rng(1).integers(0, 6, size=3 * rm.GRP, dtype=np.uint8)
    assert rm.hand_over(dense, ka, sym) == (0, 0, 0)     # nothing run-coded to start from: the run-space rebuild does not run


def _facts():
    return [(c, rm.group_facts(c[1], c[2], c[3])) for c in rm.cases()]


def test_every_border_has_a_case_on_each_side():
    claimed = {}
    wrong = []
    for c, F in _facts():
        assert c[1].size <= 5 * rm.GRP + 8 * rm.WIN, c[0]     # nothing workload-sized
        for tag in c[4]:
            if tag in rm.BORDERS:
                if rm.BORDERS[tag](F, c):
                    claimed.setdefault(tag, []).append(c[0])
                else:
                    wrong.append((c[0], tag))
    assert not wrong, "cases that are not on the border they name: %s" % wrong
    missing = sorted(set(rm.BORDERS) - set(claimed))
    assert not missing, "borders without a case: %s" % missing
    # the medium tier's ns border was reported unreachable by a probe; the table reaches it
    assert "ns13" in claimed and "ns14" in claimed and "old_words258" in rm.UNREACHABLE


def test_plane_facts_are_met():
    seen = {k: 0 for k in rm.PLANE_FACTS}
    most_words = 0
    for c, F in _facts():
        for f in F:
            most_words = max(most_words, f["nw"])
            for k, p in rm.PLANE_FACTS.items():
                seen[k] += bool(p(f))
    assert all(seen.values()), seen
    assert most_words == 257     # 258 old words cannot be reached (rm.UNREACHABLE)


def test_tiers_both_run_and_both_hand_on():
    """under reb_force 1 the table makes every counter move: small tier -> medium tier -> symbol path"""
    tot = np.zeros(3, dtype=np.int64)
    t2_only = 0
    for c, F in _facts():
        tot += rm.hand_over(c[1], c[2], c[3], facts=F)
        t2_only += sum(rm.tier(f) == 2 for f in F)
    assert tot[0] > tot[1] > 0 and tot[0] > tot[2] > 0 and t2_only >= 8, (tot, t2_only)


def _legal_moves(ka, n):
    ka = np.asarray(ka)
    nxt = np.concatenate([ka[1:], [n]])
    prv = np.concatenate([[0], ka[:-1]])
    return np.flatnonzero(ka + 1 <= nxt), np.flatnonzero(ka - 1 >= prv)


@pytest.mark.parametrize("kind", ["tie", "tie200", "geo"])
def test_cases_can_tell_a_wrong_answer(kind):
    """a case is rejected if the merged sequence does not change when the differing rows of its ties are reversed, or when no single
    insertion point moved by +1 (and by -1) changes it; a moved row is invisible only where the old symbol it passes is its own.
    The cases named *_own are all rows of the run's own symbol strictly inside it: the merged sequence is the same wherever they sit
    in the run, and what they are for is the kernel's count of items (k == nold, k == 0, a coded run start), held by the hand-over
    counters and the symbol counts on the GPU"""
    for name, old, ka, sym, _ in (c for c in rm.cases() if rm.kind_of(c[0]) == kind):
        want = rm.insert(old, ka, sym)
        n = old.size
        # reversed ties
        F = rm.group_facts(old, ka, sym)
        rev, j0, any_tie = sym.copy(), 0, False
        for f in F:
            for (a, l, k, fb, inside) in f["ties"]:
                if l >= 2 and fb >= 0:
                    seg = sym[j0 + a + fb:j0 + a + l]
                    if not np.array_equal(seg, seg[::-1]):
                        rev[j0 + a + fb:j0 + a + l] = seg[::-1]
                        any_tie = True
            j0 += f["nb"]
        if kind != "geo":
            assert any_tie or name.endswith("_own"), name       # (a tie of one symbol throughout reads the same backwards)
        if any_tie:
            assert not np.array_equal(rm.insert(old, ka, rev), want), name
        # moved insertion points: rows next to a tie border and a spread of the others
        up, down = _legal_moves(ka, n)
        in_tie = np.zeros(ka.size, dtype=bool)
        in_tie[1:] |= ka[1:] == ka[:-1]
        in_tie[:-1] |= ka[1:] == ka[:-1]
        for rows, d in ((up, 1), (down, -1)):
            rest = rows[~in_tie[rows]]
            pick = np.concatenate([rows[in_tie[rows]], rest if rest.size <= 32 else rest[np.linspace(0, rest.size - 1, 32).astype(np.int64)]])
            visible = 0
            for i in pick:
                kb = ka.copy()
                kb[i] += d
                changed = not np.array_equal(rm.insert(old, kb, sym), want)
                passed = old[ka[i]] if d == 1 else old[ka[i] - 1]
                assert changed == (passed != sym[i]), (name, int(i), d)
                visible += changed
            assert pick.size == 0 or visible > 0 or name.endswith("_own"), (name, d)


def test_model_partition_is_the_layout_models():
    for c, F in _facts():
        merged = rm.insert(c[1], c[2], c[3])
        assert len(F) == lm.n_groups(merged.size)
        assert sum(f["nsg"] for f in F) == merged.size and sum(f["nb"] for f in F) == c[2].size
        assert len(F) * lm.GRP_ALLOC + sum(f["new_slots"] for f in F) * lm.SLOT_BYTES == lm.expected_bytes_index(merged), c[0]
        ka2, sym2 = rm.second_step(merged.size)
        assert ka2[0] == 0 and ka2[-1] == merged.size and (np.diff(ka2) >= 0).all() and set(sym2.tolist()) == set(range(6))


def test_table_is_deterministic():
    rm.cases.cache_clear()
    a = [(c[0], c[1].tobytes(), c[2].tobytes(), c[3].tobytes()) for c in rm.cases()]
    rm.cases.cache_clear()
    b = [(c[0], c[1].tobytes(), c[2].tobytes(), c[3].tobytes()) for c in rm.cases()]
    assert a == b
