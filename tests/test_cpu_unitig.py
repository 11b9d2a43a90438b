"""The models of `unitig` (tests/unitig_model.py) against each other, without a GPU: the rule followed vertex by vertex, the engine's jumping rounds in numpy and brute force
on the strings agree on every set; the structural claims of DESIGN.md 7s hold; the designed set tells the rule from its near misses; and the library, the binding and
the command's usage text have the feature."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import overlap_model as om
from tests import reduce_model as rm
from tests import unitig_model as um
from tests import walk_model as wm

CLI = _build.BIN_CLI
L = um.L
_SETS, _K = um.SETS(), {}


def _kept(name):
    """a set: the strings of its rows, the lengths and the kept records of the model of `overlap --reduce` -- computed once, shared, never changed"""
    if name not in _K:
        seqs, both = _SETS[name]
        strs = om.rows_of(seqs, both)
        w = om.walk(wm.Fm(om.naive_bwt(strs)), L)
        _K[name] = dict(strs=strs, both=both, lens=w["lens"], K=w["rec"][rm.reduce_records(w["rec"], w["lens"])])
    return _K[name]


def _same(a, b):
    assert a["refused"] == b["refused"]
    for k in a:
        if k in b:
            assert np.array_equal(a[k], b[k]), k


CASES = [(name, pair) for name, (_, both) in _SETS.items() for pair in ((False, True) if both else (False,))]


@pytest.mark.parametrize("name,pair", CASES)
def test_the_restatements_agree(name, pair):
    S = _kept(name)
    a, j = um.sequential(S["K"], S["lens"], pair), um.jumping(S["K"], S["lens"], pair)
    _same(a, j)
    assert a["refused"] == (pair and name in um.ASYM)
    if pair:
        assert a["n_asym"] == um.ASYM.get(name, 0)
    if a["refused"]:
        return
    if not name.startswith("reduce"):                                            # (its 300 partners at one depth make brute force slow, and its borders are reduce_model's)
        um.brute_check(a, S["strs"], L, pair)
    # the rounds: what 7s states for the scheme that was built
    lg = lambda x: max(0, math.ceil(math.log2(max(x, 1))))    # noqa: E731
    every = um.sequential(S["K"], S["lens"], False)
    assert j["n_rounds"] <= lg(every["max_members"]) + lg(S["lens"].size) + 1
    if every["n_cycles"] == 0:
        assert j["n_rounds"] <= lg(every["max_members"]) + 1
    # the structure
    at = 0
    for h, t, n, circ, ln in a["utg"].tolist():
        mem = a["mem"][at:at + n]
        at += n
        starts, ends = mem[:, 2], mem[:, 2] + S["lens"][mem[:, 0]]
        assert (np.diff(starts) > 0).all() and (np.diff(ends) >= 0).all()       # starts strictly increase, ends never decrease
        assert ln == S["lens"][h] + int((S["lens"][mem[1:, 0]] - mem[1:, 1]).sum())
        if circ:
            assert h == mem[:, 0].min() and (not pair or h % 2 == 0)
    assert (np.diff(a["utg"][:, 0]) > 0).all()
    K, simple = S["K"], um._simple_mask(S["K"][:, :3], S["lens"].size)
    nxt = dict(zip(K[simple, 0].tolist(), K[simple, 1].tolist()))
    prv = {b: x for x, b in nxt.items()}
    heads, tails = set(every["utg"][:, 0].tolist()), set(every["utg"][:, 1].tolist())
    cyc = {h for h, _, _, c, _ in every["utg"].tolist() if c}
    for x, b in K[~simple, :2].tolist():                                         # a link goes from a tail to a head, and never touches a cycle
        assert x in tails and b in heads and x not in nxt and b not in prv
    assert not any(r in cyc for r in set(K[~simple, 0].tolist()) | set(K[~simple, 1].tolist()))
    if pair:                                                                     # chains come in mirror pairs, or are their own mirror image
        paths = {(u[0], u[1]) for u in every["utg"].tolist() if not u[3]}
        assert all((t ^ 1, h ^ 1) in paths for h, t in paths)
        assert every["n_unitigs"] == 2 * a["n_unitigs"] - sum(1 for h, t in paths if h == t ^ 1) and every["n_cycles"] == 2 * a["n_cycles"]


def test_what_the_designed_set_holds():
    S1, S2 = _kept("designed1"), _kept("designed2")
    a1, a2, b2 = um.sequential(S1["K"], S1["lens"]), um.sequential(S2["K"], S2["lens"], True), um.sequential(S2["K"], S2["lens"], False)
    w1, w2 = um.designed(both=False)[1], um.designed(both=True)[1]
    by_head = {u[0]: u for u in a1["utg"].tolist()}
    for n in um.CHAINS:
        r = w1["chain%d" % n]
        assert by_head[r[0]][1:] == [r[-1], n, 0, 60 + 10 * (n - 1)]
    r = w1["chain1000"]
    assert by_head[r[0]][1:] == [r[-1], 1000, 0, 7053] and a1["max_members"] == 1000
    assert by_head[w1["circle6"][0]][2:] == [6, 40, 160] and by_head[w1["circle2"][0]][2:] == [2, 30, 150]
    p = w1["periodic"][0]
    uid = {u[0]: i for i, u in enumerate(a1["utg"].tolist())}
    assert by_head[p][1:4] == [p, 1, 0] and [uid[p], 0, uid[p], 0, 77] in a1["links"].tolist()      # a chain of one with a link to itself
    f = w1["fork"]
    assert all(by_head[x][2] == 1 for x in f) and sorted(l for l in a1["links"].tolist() if l[0] == uid[f[0]]) == [[uid[f[0]], 0, uid[f[1]], 0, 50], [uid[f[0]], 0, uid[f[2]], 0, 50]]
    c = w1["contained"]
    assert by_head[c[0]][1:] == [c[1], 2, 0, 60] and a1["mem"][a1["mem"][:, 0] == c[1]].tolist() == [[c[1], 40, 20]]     # the tail writes no symbol
    # both strands
    by_head = {u[0]: u for u in a2["utg"].tolist()}
    mr = w2["mirror"]
    u = by_head[2 * mr[0]]
    assert u[1] == 2 * mr[0] + 1 and u[2] == 16 and u[4] == 140                  # all 16 rows on one chain with h == t ^ 1, output once
    assert a2["n_cycles"] == 2 and b2["n_cycles"] == 4                           # of the two cycles of a circle exactly one is output
    f = [2 * x for x in w2["fork"]]
    fork_all = [l for l in b2["links"].tolist() if l[4] == 50]
    uid = {u[0]: i for i, u in enumerate(a2["utg"].tolist())}
    assert len(fork_all) == 4 and sorted(l for l in a2["links"].tolist() if l[4] == 50) == [[uid[f[0]], 0, uid[f[1]], 0, 50], [uid[f[0]], 0, uid[f[2]], 0, 50]]
    assert a2["n_links"] == 3 and sorted(x[4] for x in a2["links"].tolist()) == [50, 50, 77]
    # the random reads: what the prototype found
    for name, pair, links in (("reads1", False, 28), ("reads2", True, 28), ("reads2", False, 56)):
        S = _kept(name)
        a = um.sequential(S["K"], S["lens"], pair)
        assert (a["n_unitigs"], a["n_symbols"], a["max_members"], a["n_links"]) == (46 if name == "reads2" and not pair else 23, 4804 if name == "reads2" and not pair else 2402, 50, links)


def test_the_near_misses_are_told_apart():
    S1, S2 = _kept("designed1"), _kept("designed2")
    for S, pair, switches in ((S1, False, ("self_loops", "cut_largest")), (S2, True, ("self_loops", "cut_largest", "strict_mirror"))):
        a = um.sequential(S["K"], S["lens"], pair)
        for sw in switches:
            b = um.sequential(S["K"], S["lens"], pair, **{sw: True})
            assert not all(np.array_equal(a[k], b[k]) for k in ("utg", "mem", "links")), sw
    b = um.sequential(S2["K"], S2["lens"], True, strict_mirror=True)              # h < t ^ 1 loses the self-mirror path
    assert b["n_unitigs"] == um.sequential(S2["K"], S2["lens"], True)["n_unitigs"] - 1
    # degrees per partner instead of per record: two records between the same two strings at two depths
    t = np.tile(np.array([1, 2, 3, 4, 1, 1, 2], dtype=np.uint8), 3)
    strs = [np.concatenate([np.array([4, 4, 3, 2, 4, 3, 3, 1], dtype=np.uint8), t[:14]]), np.concatenate([t[:14], np.array([2, 2, 2, 4, 4, 1, 3, 4], dtype=np.uint8)])]
    w = om.walk(wm.Fm(om.naive_bwt(strs)), 5)
    K = w["rec"][rm.reduce_records(w["rec"], w["lens"])]
    ab = [x[:2] for x in K.tolist()]
    assert ab.count([0, 1]) == 2                                                 # (0, 1, 14) and (0, 1, 7): neither implies the other
    a, b = um.sequential(K, w["lens"]), um.sequential(K, w["lens"], per_partner=True)
    assert a["n_simple"] == 0 and a["n_unitigs"] == 2 and a["n_links"] == 2 and b["n_simple"] == 2


def test_library_exports_unitigs():
    lib = ctypes.CDLL(_build.LIB_GPU)
    assert hasattr(lib, "rb3gpu_unitigs")
    from ropebwt3_amd import gpu
    assert "rb3gpu_unitigs" in gpu.SYMBOLS and ctypes.sizeof(gpu.UnitigStats) == 5 * 8 + 14 * 8 and hasattr(gpu.Rb3Gpu, "unitigs")
    assert [k for k, _ in gpu.UnitigStats._fields_] == ["ms_total", "ms_reduce", "ms_graph", "ms_rank", "ms_emit", "n_strings", "n_kept", "n_simple", "n_unitigs", "n_members",
                                                        "n_symbols", "n_steps_emit", "n_cycles", "n_asym", "n_links", "n_rounds", "max_members", "n_slices", "resident_bytes"]
    assert gpu.UNITIG_REC.itemsize == 24 and gpu.UNITIG_MEMBER.itemsize == 16 and gpu.UNITIG_LINK.itemsize == 16


def test_usage_lists_unitig():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"unitig" in r.stdout + r.stderr
    r = subprocess.run([CLI, "unitig"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and all(x in r.stderr for x in (b"--pair", b"--gfa", b"--table", b"-l INT", b"-c INT"))
