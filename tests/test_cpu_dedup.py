"""`dedup` without a GPU: the walk restated over tests/walk_model.Fm (tests/dedup_model.py) against brute force on the strings themselves -- on every committed plain
BWT and on a designed set that holds every case the rule names --, and what the library and the command line must offer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import dedup_model as dm
from tests import kount_model as km
from tests import util
from tests import walk_model as wm

CLI = _build.BIN_CLI
GOLDEN = util.GOLDEN
PLAIN = ["edge_dups", "edge_chars", "k2_fwd", "k3_both", "k4_readme", "reads_fwd", "reads_fq", "genomes12"]
BOTH = {"edge_dups", "edge_chars", "k3_both", "k4_readme", "reads_fq", "genomes12"}      # built from both strands, in input order

_FM = {}


def _fm(name):
    """(Fm, the strings of its rows): computed once, shared, never changed"""
    if name not in _FM:
        fm = wm.Fm(km.read_plain(os.path.join(GOLDEN, name + ".bwt.gz")))
        strs = fm.retrieve(np.arange(int(fm.acc[1])))[1]
        _FM[name] = (fm, strs, dm.Brute(strs))
    return _FM[name]


def _same(fm, bf, pair):
    """the model, with and without the early exit, against brute force"""
    full, steps_full, none = dm.walk(fm, early=False)
    fast, steps_fast, n_early = dm.walk(fm, early=True)
    assert none == 0 and steps_full == fm.n                 # every row of the index is read once
    assert steps_fast <= steps_full and (n_early > 0) == (steps_fast < steps_full)
    gone = fast[:, 2] < 0
    assert int(gone.sum()) == n_early and (full[gone, 0] == 1).all() and (full[gone, 1] == 1).all() and np.array_equal(full[~gone], fast[~gone])
    for dup_only in (False, True):
        want = bf.kinds(pair, dup_only)
        for rec in (full, fast):
            kind, keeper = dm.kinds(rec, pair, dup_only)
            assert np.array_equal(kind, want[0]) and np.array_equal(keeper, want[1]), (pair, dup_only)
    return full, bf.kinds(pair, False)


@pytest.mark.parametrize("name", PLAIN)
def test_model_against_brute_force_on_the_committed_indexes(name):
    fm, strs, bf = _fm(name)
    m = len(strs)
    assert m <= 7000
    for pair in ((False, True) if name in BOTH else (False,)):
        if pair:
            assert all(np.array_equal(util.revcomp(strs[r]), strs[r + 1]) for r in range(0, m, 2))
        full, _ = _same(fm, bf, pair)
        assert np.array_equal(full[:, 1], bf.copies)
        assert np.array_equal(full[:, 0], bf.occ)            # (brute force counts every place in one scan per distinct string: cheap enough above 700 strings too)
        assert np.array_equal(full[:, 0] > full[:, 1], bf.inside)                      # occ > copies iff the string lies inside a longer one
    if name == "reads_fq":
        assert int((full[:, 1] > 1).sum()) == 314
    if name == "edge_dups":
        kind = dm.kinds(full, False, False)[0]
        assert int((kind == dm.C).sum()) == 6 and int((full[:, 1] > 1).sum()) == 6


def test_pair_on_one_strand_is_refused_by_the_model():
    fm = _fm("reads_fwd")[0]
    rec = dm.walk(fm)[0]
    with pytest.raises(ValueError):
        dm.kinds(rec, pair=True)                             # an even number of rows that are nobody's strands
    fm = _fm("k4_readme")[0]
    with pytest.raises(ValueError):
        dm.kinds(dm.walk(fm)[0][:1], pair=True)              # an odd number of rows


@pytest.mark.parametrize("both", [False, True])
def test_model_against_brute_force_on_the_designed_set(both):
    seqs = dm.designed(both=both)
    strs = dm.rows_of(seqs, both)
    b = dm.naive_bwt(strs)
    fm = wm.Fm(b)
    assert b.size == sum(s.size + 1 for s in strs) and all(np.array_equal(x, y) for x, y in zip(fm.retrieve(np.arange(len(strs)))[1], strs))
    assert np.array_equal(b, util.Oracle().bwt(util.make_text(seqs, rev=both)))       # the naive sort is the index's order
    bf = dm.Brute(strs)
    full, (kind, keeper) = _same(fm, bf, both)
    occ, copies = bf.occ, bf.copies
    assert np.array_equal(full[:, 0], occ) and np.array_equal(full[:, 1], copies)
    for k in (dm.K, dm.D, dm.C):
        assert int((kind == k).sum()) >= 8, chr(k)
    if both:
        assert b.size > 2 * 8192                             # ranks cross group borders
    else:
        assert any(s.size == 0 for s in strs) and occ[[s.size for s in strs].index(0)] == b.size
    # what the set was designed to hold, as brute force sees it
    rows = [s.tobytes() for s in strs]
    unit = (lambda r: r >> 1) if both else (lambda r: r)
    pal = [r for r, s in enumerate(strs) if s.size > 2 and np.array_equal(s, util.revcomp(s))]
    assert len({rows[r] for r in pal}) == 2
    if both:
        assert all(kind[unit(r)] == dm.K for r in pal if copies[r] == 2)              # a palindrome alone keeps itself
        rc_only = [u for u in range(len(seqs)) if kind[u] == dm.D and rows[0::2].count(rows[2 * u]) == 1]
        assert rc_only                                                                # a duplicate only through somebody's reverse complement
    assert rows.count(bytes([5, 5])) == (2 if both else 1)
    one_off = [r for r, s in enumerate(strs) if s.size == 77]
    assert len(one_off) == (6 if both else 3) and all(kind[unit(r)] == dm.K for r in one_off)
    assert dm.drop_text(kind) == b"".join(b"%d\n" % u for u in range(len(kind)) if kind[u] != dm.K)


def test_early_exit_costs_the_logarithm():
    """unrelated reads: a suffix of L random symbols occurs at another of the n places with probability about n / 4^L, so a walk ends after about log4(n) steps and
    a few -- not after its length.  (Reads that overlap, as those of reads_fwd do, share their suffixes until one of them ends: there the exit comes later.)"""
    rng = np.random.default_rng(3)
    strs = [util.random_genome(rng, 100) for _ in range(300)]
    fm = wm.Fm(dm.naive_bwt(strs))
    rec, steps, n_early = dm.walk(fm, early=True)
    assert n_early == len(strs) and (rec == (1, 1, -1)).all()
    assert steps <= len(strs) * (np.log(fm.n) / np.log(4) + 4) < 0.2 * fm.n
    fm, strs, _ = _fm("reads_fwd")
    assert dm.walk(fm, early=True)[1] < dm.walk(fm, early=False)[1] == fm.n


def test_library_exports_dedup():
    lib = ctypes.CDLL(_build.LIB_GPU)
    assert hasattr(lib, "rb3gpu_dedup")
    from ropebwt3_amd import gpu
    assert "rb3gpu_dedup" in gpu.SYMBOLS and ctypes.sizeof(gpu.DedupStats) == 2 * 8 + 7 * 8 and hasattr(gpu.Rb3Gpu, "dedup")
    assert gpu.DEDUP_REC.itemsize == 24


def test_usage_lists_dedup():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and any(line.split()[:1] == [b"dedup"] for line in r.stdout.splitlines())
    r = subprocess.run([CLI, "dedup"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and all(w in r.stderr for w in (b"dedup", b"--pair", b"--dup-only", b"--table"))
