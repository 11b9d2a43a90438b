"""The GPU suffix sorter's restatement (tests/sort_model.py) against the definition and the host sorter, and the proof that the committed
inputs reach the borders of k_s_wsort, of the depth rule and of the key width that tests/test_gpu_sort.py runs on the device.  No GPU."""
import functools

import numpy as np
import pytest

from tests import sort_model as sm
from tests import util

FX = sm.fixtures()
SMALL = [k for k, t in FX.items() if t.size <= 20000]


@functools.lru_cache(maxsize=None)
def brute(name):
    return sm.brute_sa(FX[name])


def _spans(c):
    return c["span_1"] + c["span_2_64"] + c["span_65_126"] + c["span_127"]


@pytest.mark.parametrize("name", SMALL)
def test_model_is_the_definition(name):
    m = sm.model(name)
    assert np.array_equal(m.sa, brute(name))
    assert np.array_equal(m.sa[m.isa], np.arange(m.n)) and np.array_equal(m.tw >> np.uint64(3), m.isa.astype(np.uint64))


@pytest.mark.parametrize("name", list(FX))
def test_model_bwt_is_the_host_sorters(name):
    from ropebwt3_amd import host
    assert np.array_equal(sm.model(name).bwt, host.build_bwt(FX[name]))


@pytest.mark.parametrize("name", list(FX))
def test_inner_walkers_are_ckrow_entries(name):
    """the walkers strictly inside strings carry rows of the sampled inverse suffix array (the host takes steps from 2 on)"""
    from ropebwt3_amd import host
    m = sm.model(name)
    for step in (7, 100):
        _, w = host.build_bwt_walkers(FX[name], step)
        inner = w[w[:, 1] == -1]
        ck = m.ckrow(step)
        assert ck.size == (m.n + step - 1) // step and set(inner[:, 0].tolist()) <= set(ck.tolist())


@pytest.mark.parametrize("c", sm.FAMILY)
def test_census_family(c):
    """groups of exactly c members that need a real reordering.  A group of 65..127 members is LARGE only where it starts so late in its
    chunk that it ends behind the next one (lane > 127 - size): in family_65 the 32 groups of a round follow each other from lane 0 on
    and none starts at lane 63, so all of them are wave-sorted in spans of 65..126 -- copies_65 has the large group of 65."""
    m = sm.model("family_%d" % c)
    cs = m.census
    print("family_%d" % c, m.rounds, cs, m.per_round)
    assert cs["largest"] == c and m.rounds == 2
    if c <= 64:
        assert cs["flag_large"] == 0 and cs["to_device_sort"] == 0
    if c == 65:
        assert cs["flag_large"] == 0 and cs["span_65_126"] > 0
    if c == 127:
        assert cs["span_127"] >= 1
    if c > 65:
        assert cs["mixed_rounds"] >= 1
    if c >= 128:
        assert cs["to_device_sort"] >= c


@pytest.mark.parametrize("c", sm.COPIES)
def test_census_copies(c):
    """every group has exactly c members in every round; the sentinel order decides"""
    m = sm.model("copies_%d" % c)
    cs = m.census
    print("copies_%d" % c, m.rounds, cs, m.per_round)
    assert cs["largest"] == c and m.rounds == 3
    n_chunks = cs["skipped"] + cs["end_in_chunk"] + cs["end_in_next"] + cs["flag_large"]
    if c == 64:     # every chunk starts a group at lane 0 and ends on the head (or the list end) at position 64
        assert cs["skipped"] == 0 and cs["flag_large"] == 0 and cs["end_in_next"] == n_chunks == cs["span_2_64"]
    if c == 65:     # a group of 65 at lane 63 is large, beside wave-sorted ones
        assert cs["flag_large"] >= 1 and cs["mixed_rounds"] >= 1 and cs["span_65_126"] > 0
    if c == 127:
        assert cs["span_127"] >= 1 and cs["mixed_rounds"] == m.rounds
    if c >= 128:    # every group large: no wave sorts anything
        assert _spans(cs) == 0 and cs["flag_large"] > 0 and cs["flag_large"] + cs["skipped"] == n_chunks
        assert cs["to_device_sort"] == c * cs["flag_large"]
    if c < 65:
        assert cs["flag_large"] == 0


def test_census_mix_and_both_strands():
    m = sm.model("mix")
    cs = m.census
    print("mix", m.rounds, cs, m.per_round)
    assert m.rounds == 2 and all(wave > 0 and large > 0 for wave, large in m.per_round)
    assert cs["span_127"] >= 1 and cs["skipped"] > 100 and cs["largest"] == sum(sm.MIX)    # (the sentinels: one group in round 1)
    for name, largest in (("both_family_129", 258), ("both_copies_65", 130)):
        m = sm.model(name)
        print(name, m.rounds, m.census, m.per_round)
        assert m.census["largest"] == largest and m.census["mixed_rounds"] >= 1
        z = np.flatnonzero(FX[name] == 0)                     # reverse-complement strings interleaved
        assert np.array_equal(FX[name][z[0] + 1:z[1]], util.revcomp(FX[name][:z[0]]))


@pytest.mark.parametrize("L,rounds,h0", [(1, 0, 20), (19, 0, 20), (20, 0, 20), (21, 1, 20), (39, 1, 20), (40, 1, 20), (41, 2, 20), (4095, 8, 20), (4096, 8, 16), (4097, 9, 16)])
def test_depth_rule_and_key_width_borders(L, rounds, h0):
    """one string of L times A: the suffixes at d == h - 1, h, h + 1 of every round, and n / n_strings == 4096 and 4097"""
    m = sm.model("homopolymer_%d" % L)
    print("homopolymer_%d" % L, m.rounds, m.census, m.per_round)
    assert (m.rounds, m.h0) == (rounds, h0)
    if L >= 4095:
        assert m.per_round[:8] == [(0, 1)] * 8     # one large group per round


def test_census_small_ends():
    m = sm.model("singles")
    print("singles", m.rounds, m.census, m.per_round)
    assert m.rounds == 1 and m.census["end_in_chunk"] == 1 and _spans(m.census) == 1 and m.census["largest"] == 8
    assert sm.model("one_symbol").rounds == 0
    a, b = sm.model("len4095x3"), sm.model("len4096x3")
    print("len4095x3", a.rounds, a.census, "len4096x3", b.rounds, b.census)
    assert (a.h0, b.h0) == (20, 16) and a.census["largest"] == b.census["largest"] == 3     # the string, its mutant, its copy


# one rule of the model swapped for a wrong copy -> the (smallest) fixture whose suffix array it spoils
CAUGHT = {"sid0": "singles", "index": "homopolymer_41", "nocut": "singles"}


def _spoils(name, broken):
    try:
        return not np.array_equal(sm.sort(FX[name], broken=broken).sa, brute(name))
    except AssertionError:     # more than 40 rounds: no answer at all
        return True


@pytest.mark.parametrize("broken", sorted(CAUGHT))
def test_fixtures_tell_a_broken_rule(broken):
    """the inputs tell right from wrong, on the model's side (nothing on the GPU is mutated):
      sid0    the string number replaced by 0: `singles` (A$ three times: the sub-group never splits, no answer after 40 rounds); every
              copies_* and family_* fixture too
      index   the new rank from the element's own index: `homopolymer_41` (a tied sub-group falls apart into groups of one and is never
              put in order); every fixture that needs a second round for a tie
      nocut   h0 symbols compared past the sentinel: `singles` (the sixth string's A$A.. goes before the first string's A$C..: the next string decides, not the string number)"""
    assert _spoils(CAUGHT[broken], broken)
    assert sum(_spoils(k, broken) for k in SMALL) >= 3


@pytest.mark.parametrize("broken", ["le", "reverse"])
def test_rules_no_input_can_tell(broken):
    """two of the rules the sorter could get 'wrong' cannot spoil a suffix array, so no fixture can catch them -- pinned here as such:
      le       d <= h instead of d < h.  At d == h the right key is rank[p + h], the rank of p's own sentinel: 0 while the sentinels are one
               group (round 1), the string number afterwards.  The string number is below n_strings, every rank of a suffix that does not
               start with a sentinel is at least n_strings, and the members of a group with d == h differ from each other in nothing
               but their sentinels: the same order, at most one round earlier.
      reverse  ties (equal second rank) reversed inside a sub-group.  A sub-group of several members stays in the list with one rank
               for all, is one group of the next round whatever the order of its members, and its slots are written again then.
    The model agrees with the definition on every fixture under either, and takes no more rounds."""
    for name in SMALL:
        m = sm.sort(FX[name], broken=broken)
        assert np.array_equal(m.sa, brute(name)) and m.rounds <= sm.model(name).rounds, name
