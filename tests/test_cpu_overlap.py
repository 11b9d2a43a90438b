"""`overlap` without a GPU: the walk restated over tests/walk_model.Fm (tests/overlap_model.py) against brute force on the strings themselves -- on every committed
plain BWT small enough for brute force and on a designed set that holds every case --, and what the library and the command line must offer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import kount_model as km
from tests import overlap_model as om
from tests import util
from tests import walk_model as wm

CLI = _build.BIN_CLI
GOLDEN = util.GOLDEN
# every committed plain BWT but genomes12 (24 strings of 20 000 symbols: 4.8 G bytes of prefixes), each with a minimum length of 1, a middle one and one above every
# string -- reads_fq from 12 on: at 1 its 6104 strings have 12 M records, too many for sets of Python tuples
PLAIN = {"edge_dups": (1, 3, 6), "edge_chars": (1, 10, 42), "k2_fwd": (1, 2, 4), "k3_both": (1, 2, 4), "k4_readme": (1, 10, 32), "reads_fwd": (1, 31, 101),
         "reads_fq": (12, 50, 101)}
BOTH = {"edge_dups", "edge_chars", "k3_both", "k4_readme", "reads_fq"}      # built from both strands, in input order

_SET = {}


def _designed(both):
    """the designed set: its strings, its index and brute force on it -- computed once, shared, never changed"""
    if both not in _SET:
        seqs = om.designed(both=both)
        strs = om.rows_of(seqs, both)
        b = om.naive_bwt(strs)
        _SET[both] = dict(seqs=seqs, strs=strs, b=b, fm=wm.Fm(b), bf=om.Brute(strs))
    return _SET[both]


def _same(fm, bf, min_len, max_len):
    """the model, with and without the early exit, against brute force: the same set, no record twice, the engine's order; returns the records"""
    want = bf.triples(min_len)
    full, fast = om.walk(fm, min_len, 0, early=False), om.walk(fm, min_len, 0, early=True)
    assert om.triples(full["rec"]) == want and np.array_equal(full["rec"], fast["rec"]), min_len
    assert full["n_early"] == 0 and full["steps_count"] == fm.n                     # every row of the index is read once
    assert fast["steps_count"] <= fm.n and (fast["n_early"] > 0) == (fast["steps_count"] < fm.n)
    for w in (full, fast):
        rec = w["rec"]
        assert w["n_capped_groups"] == 0 and int(w["cnt"].sum()) == rec.shape[0] and w["steps_emit"] == int((w["last"] + 1)[w["cnt"] > 0].sum())
        if rec.shape[0]:
            key = rec[:, 0] * (max_len + 1) + (max_len - rec[:, 2])                 # a ascending, then len descending
            assert (np.diff(key) >= 0).all() and (rec[:, 2] >= min_len).all() and (rec[:, 2] < w["lens"][rec[:, 0]]).all() and (rec[:, 2] <= rec[:, 3]).all()
            assert np.array_equal(rec[:, 3], w["lens"][rec[:, 1]])
            assert np.array_equal(np.bincount(rec[:, 0], minlength=w["cnt"].size), w["cnt"]) and np.array_equal(w["last"][w["cnt"] > 0], _first_len(rec))
    return full["rec"]


def _first_len(rec):
    """the len of the first record of every a: the longest, as the records are ordered"""
    first = np.flatnonzero(np.concatenate([[True], np.diff(rec[:, 0]) != 0]))
    return rec[first, 2]


def _mirrored(rec):
    """on both strands (a, len, b) is there iff (b ^ 1, len, a ^ 1) is -- except where len is the whole of b (or, seen from the other side, of a, which no record has)"""
    got = om.triples(rec)
    lens = {}
    for a, b, l, lb in rec.tolist():
        lens[b] = lb
    n = 0
    for a, l, b in got:
        if l < lens[b]:
            assert (b ^ 1, l, a ^ 1) in got, (a, l, b)
            n += 1
    return n


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_model_against_brute_force_on_the_committed_indexes(name):
    fm = wm.Fm(km.read_plain(os.path.join(GOLDEN, name + ".bwt.gz")))
    strs = fm.retrieve(np.arange(int(fm.acc[1])))[1]
    longest = max(s.size for s in strs)
    assert sum(s.size ** 2 for s in strs) <= 10 ** 8
    bf = om.Brute(strs)
    lo, mid, hi = PLAIN[name]
    assert lo < mid < longest < hi
    for min_len in (lo, mid, hi):
        rec = _same(fm, bf, min_len, longest)
        assert rec.shape[0] == 0 if min_len == hi else rec.shape[0] > 0 or name in ("k2_fwd", "k4_readme")    # (two strings each, and no end that starts the other)
        if name in BOTH:
            _mirrored(rec)
    assert np.array_equal(om.who_of(fm)[1], [s.size for s in strs])


@pytest.mark.parametrize("both", [False, True])
def test_model_against_brute_force_on_the_designed_set(both):
    S = _designed(both)
    strs, b, fm, bf = S["strs"], S["b"], S["fm"], S["bf"]
    assert b.size > 2 * 8192                                                       # ranks cross group borders
    assert all(np.array_equal(x, y) for x, y in zip(fm.retrieve(np.arange(len(strs)))[1], strs))
    assert np.array_equal(b, util.Oracle().bwt(util.make_text(S["seqs"], rev=both)))   # the naive sort is the index's order
    longest = max(s.size for s in strs)
    L = om.MIN_LEN
    recs = {min_len: _same(fm, bf, min_len, longest) for min_len in (1, L, longest + 1)}
    assert recs[longest + 1].shape[0] == 0 and recs[1].shape[0] > 50 * recs[L].shape[0] > 0
    rec = recs[L]
    if both:
        assert 0 < _mirrored(rec) < rec.shape[0] and _mirrored(recs[1]) > 0
    # what the set was designed to hold, as brute force sees it
    rows = [s.tobytes() for s in strs]
    groups = bf.groups(L)
    sizes = sorted(groups.values())
    assert sizes.count(8) == 1 and sizes.count(om.CAP) == 1 and sizes.count(om.CAP + 1) == 1 and sizes[-1] == 300 and sizes[-2] == om.CAP + 1
    got = bf.triples(L)
    lens = [len(r) for r in rows]
    assert any(l == L and lens[a] == 60 and lens[b_] == L + 40 for a, l, b_ in got)                       # exactly the minimum
    assert any(l == L - 1 and lens[a] == 60 and lens[b_] == L - 1 + 40 for a, l, b_ in bf.triples(L - 1))  # one below it: there,
    assert not any(lens[a] == 60 and lens[b_] == L - 1 + 40 for a, l, b_ in got)                          # ... and not at the minimum
    assert any(l == lens[a] - 1 for a, l, b_ in got) and any(l == lens[b_] for a, l, b_ in got)
    per = [a for a in range(len(rows)) if lens[a] == 84 and rows[a][:7] * 12 == rows[a]]
    assert per and {l for a, l, b_ in got if a == per[0] and b_ == per[0]} == set(range(21, 84, 7))       # self-overlaps at every multiple of the period
    assert any(5 in rows[a][lens[a] - l:] for a, l, b_ in got)                     # an N inside an overlap
    ties = [(a, l) for a, l, b_ in got for b2 in (b_ + (2 if both else 1),) if (a, l, b2) in got and rows[b_] == rows[b2]]
    assert ties                                                                    # exact copies among the partners of one group
    assert 1 in lens and (0 in lens) == (not both)
    if both:
        assert any(a ^ 1 == b_ for a, l, b_ in got)                                # a suffix that starts the string's own reverse complement
        assert any(np.array_equal(util.revcomp(s[:25]), s[-25:]) for s in strs if s.size == 70)
    # the cap: of the groups at MIN_LEN two are over CAP -- the one of CAP + 1 and the one of 300 partners --, 1.1 % of the 182 groups on one strand
    capped = [z for z in groups.values() if z > om.CAP]
    assert len(capped) == 2 and sum(capped) == om.CAP + 1 + 300 and len(capped) <= 0.02 * len(groups)
    for early in (False, True):
        w = om.walk(fm, L, om.CAP, early)
        assert w["n_capped_groups"] == 2 and w["n_capped_hits"] == om.CAP + 1 + 300 and w["n_groups"] == len(groups) - 2
        assert om.triples(w["rec"]) == {(a, l, b_) for a, l, b_ in got if groups[(a, l)] <= om.CAP} and w["rec"].shape[0] == len(got) - sum(capped)
    w1 = om.walk(fm, L, 1, True)                                                   # a cap of one: only the overlaps nobody shares
    assert om.triples(w1["rec"]) == {(a, l, b_) for a, l, b_ in got if groups[(a, l)] == 1}
    # the slices of the emit stage
    cnt = om.walk(fm, L, 0, True)["cnt"]
    assert om.slices(cnt, 1) == cnt[cnt > 0].tolist() and sum(om.slices(cnt, 64)) == int(cnt.sum()) and max(om.slices(cnt, 64)) == 300
    assert all(t <= 64 for t in om.slices(cnt, 64) if t != 300) and len(om.slices(cnt, 10 ** 9)) == 1 and om.slices(cnt * 0, 5) == []


def test_the_commands_bytes():
    rec = np.array([[0, 3, 25, 40], [5, 4, 7, 7]], dtype=np.int64)
    lens = np.array([30, 0, 0, 40, 7, 9], dtype=np.int64)
    assert om.text(rec, lens) == b"0\t3\t25\t30\t40\n5\t4\t7\t9\t7\n"
    assert om.text(rec, lens, pair=True) == b"0\t+\t1\t-\t25\t30\t40\n2\t-\t2\t+\t7\t9\t7\n"
    assert om.text(rec[:0], lens) == b""


def test_library_exports_overlap():
    lib = ctypes.CDLL(_build.LIB_GPU)
    assert hasattr(lib, "rb3gpu_overlap")
    from ropebwt3_amd import gpu
    assert "rb3gpu_overlap" in gpu.SYMBOLS and ctypes.sizeof(gpu.OverlapStats) == 4 * 8 + 10 * 8 and hasattr(gpu.Rb3Gpu, "overlap")
    assert gpu.OVERLAP_REC.itemsize == 16 and gpu.OVERLAP_REC.names == ("a", "b", "len", "len_b")


def test_usage_lists_overlap():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and any(line.split()[:1] == [b"overlap"] for line in r.stdout.splitlines())
    r = subprocess.run([CLI, "overlap"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and all(w in r.stderr for w in (b"overlap", b"-l INT", b"-c INT", b"--pair", b"--gpu"))
