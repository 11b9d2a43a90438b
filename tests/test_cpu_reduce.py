"""`overlap --reduce` without a GPU: the rule on the records against brute force on the strings (tests/reduce_model.py) -- on the designed set that holds every border of
the rule, on the designed set of `overlap`, on random reads --, the rule and what follows from it on the committed plain BWTs, the cap, the near misses of the rule that
the designed set must tell from it, and what the library and the command line must offer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import kount_model as km
from tests import overlap_model as om
from tests import reduce_model as rm
from tests import util
from tests import walk_model as wm

CLI = _build.BIN_CLI
L, CAP = om.MIN_LEN, om.CAP
# the committed plain BWTs of tests/test_cpu_overlap.py with its minimum lengths: 1, a middle one and one above every string -- the two read sets from 12 on (at 1
# the 1000 strings of reads_fwd have 335 k records and 56 M pairs of them to try: seconds of numpy for borders the smaller sets hold already)
PLAIN = {"edge_dups": (1, 3, 6), "edge_chars": (1, 10, 42), "k2_fwd": (1, 2, 4), "k3_both": (1, 2, 4), "k4_readme": (1, 10, 32), "reads_fwd": (12, 31, 101),
         "reads_fq": (12, 50, 101)}
BOTH = {"edge_dups", "edge_chars", "k3_both", "k4_readme", "reads_fq"}      # built from both strands, in input order

_SET = {}


def _index(name, both):
    """a set of sequences as rows, BWT and model index -- computed once, shared, never changed"""
    if (name, both) not in _SET:
        seqs = {"reduce": rm.designed_reduce, "overlap": om.designed}[name](both=both) if name != "reads" else rm.read_set()
        strs = om.rows_of(seqs, both)
        _SET[(name, both)] = dict(strs=strs, fm=wm.Fm(om.naive_bwt(strs)))
    return _SET[(name, both)]


def _kept(w, keep):
    return {(int(a), int(l), int(b)) for (a, b, l, _), k in zip(w["rec"].tolist(), keep.tolist()) if k}


def _by_sets(rec, lens, overhang=True):
    """the rule on the records once more, on a Python set of triples and nothing else: the keep mask"""
    R = {(a, b, o) for a, b, o, _ in rec.tolist()}
    by_a = {}
    for a, c, oc, _ in rec.tolist():
        by_a.setdefault(a, []).append((c, oc))
    return np.array([not any(oc > o and (lens[c] > oc or not overhang) and (c, b, int(lens[c]) - oc + o) in R for c, oc in by_a[a]) for a, b, o, _ in rec.tolist()], dtype=bool)


def _consequences(w, keep, both):
    """what follows from the rule: the deepest group of every string is kept whole, so the strings with kept records are the strings with records; on both strands a
    record is kept iff its mirror image is, wherever both are records -- but for one border.  Under the mirror the conditions len(c) > o_c and o' < len(b) change
    places, and the second is part of what a record is only on the mirror's side: where EVERY witness of (a, b, o) has o' == len(b) -- b ends where c ends, which the rule
    counts -- the mirror image has no witness, because rc(b) as a whole is no overlap with rc(c).  Such a b is contained in c: after `dedup | remove` there is none.
    (That the kept records are a subsequence is what a mask says.)  Returns the mirror pairs that agree and those at the border"""
    rec, lens = w["rec"], w["lens"]
    if rec.shape[0] == 0:
        return 0, 0
    first = np.concatenate([[True], np.diff(rec[:, 0]) != 0])
    deepest = rec[:, 2] == np.repeat(rec[first, 2], np.diff(np.concatenate([np.flatnonzero(first), [rec.shape[0]]])))
    assert keep[deepest].all()
    assert np.array_equal(np.unique(rec[keep, 0]), np.unique(rec[:, 0])) and np.array_equal(np.unique(rec[:, 0]), np.flatnonzero(w["cnt"] > 0))
    n = border = 0
    if both:
        state = {(a, l, b): k for (a, b, l, _), k in zip(rec.tolist(), keep.tolist())}
        by_a = {}
        for a, l, c in state:
            by_a.setdefault(a, []).append((c, l))
        for (a, l, b), k in state.items():
            if (b ^ 1, l, a ^ 1) not in state:
                continue
            if state[(b ^ 1, l, a ^ 1)] == k:
                n += 1
            elif not k:                                                      # reduced, its mirror image kept: every witness ends where b ends
                wit = [(c, oc) for c, oc in by_a[a] if oc > l and lens[c] > oc and (c, int(lens[c]) - oc + l, b) in state]
                assert wit and all(int(lens[c]) - oc + l == lens[b] for c, oc in wit), (a, l, b)
                border += 1
    return n, border


def _agree(S, min_len, both):
    """both models on one set: the same records and the same kept ones; returns the walk, the mask and the two sets of brute force"""
    w = om.walk(S["fm"], min_len)
    keep = rm.reduce_records(w["rec"], w["lens"])
    kept, every = rm.reduce_strings(S["strs"], min_len)
    assert om.triples(w["rec"]) == every and _kept(w, keep) == kept
    assert np.array_equal(keep, _by_sets(w["rec"], w["lens"]))
    _consequences(w, keep, both)
    return w, keep, kept, every


@pytest.mark.parametrize("both", [False, True])
def test_models_agree_on_the_designed_set(both):
    S = _index("reduce", both)
    w, keep, kept, every = _agree(S, L, both)
    assert 0 < int(keep.sum()) < keep.size and w["cnt"].max() > 300                      # a list of more than 300 records
    lists = {}
    for a, b, l, _ in w["rec"].tolist():
        lists.setdefault(a, []).append((l, b))
    for name, c in rm.designed_cases().items():
        if c["strand"] and not both:
            continue
        a, wit = rm.row(c["a"], both), rm.row(c["c"], both)
        bs, ks = (c["b"], c["kept"]) if name == "big" else ([c["b"]], [c["kept"]])
        for b, k in zip(bs, ks):
            t = (a, c["o"], rm.row(b, both, c["strand"]))
            assert t in every and (t in kept) == k, (name, t)
        if "list" in c:                                                                  # the ends of the binary search: the size of c's list and the target's place
            size, place = c["list"]
            o_c = max(l for l, x in lists[a] if x == wit)
            target = (S["strs"][wit].size - o_c + c["o"], rm.row(c["b"], both))
            got = lists.get(wit, [])
            assert len(got) == size and (got.index(target) if target in got else None) == place, (name, got, target)
    cs = rm.designed_cases()
    both_copies = [(rm.row(cs["witness_copies"]["a"], both), 40, rm.row(cs["witness_copies"][x], both)) for x in ("c", "c2")]
    assert all(t in kept for t in both_copies)                                           # neither copy of a witness is longer than the other
    s = rm.row(cs["periodic"]["a"], both)
    assert {l for a, l, b in every if a == s and b == s} == set(range(21, 84, 7)) and {l for a, l, b in kept if a == s and b == s} == {77}
    if both:
        n, border = _consequences(w, keep, both)
        assert n > 100 and border >= 1                                                   # ends_with_c: reduced, its mirror image kept


def test_designed_set_tells_the_rule_from_its_near_misses():
    S = _index("reduce", False)
    w = om.walk(S["fm"], L)
    cs = rm.designed_cases()
    kept, every = rm.reduce_strings(S["strs"], L)
    t = (cs["suffix_only"]["a"], 25, cs["suffix_only"]["b"])
    # condition 2 dropped: a witness that is only a suffix of a reduces the record, in both models
    loose = rm.reduce_strings(S["strs"], L, overhang=False)[0]
    assert t in kept and t not in loose and loose < kept
    assert _kept(w, rm.reduce_records(w["rec"], w["lens"], overhang=False)) == loose
    assert np.array_equal(rm.reduce_records(w["rec"], w["lens"], overhang=False), _by_sets(w["rec"], w["lens"], overhang=False))
    # o_c > o weakened to >=: on the strings every partner longer than the overlap becomes its own witness
    weak = rm.reduce_strings(S["strs"], L, strict=False)[0]
    t = (cs["below_min"]["a"], L, cs["below_min"]["b"])
    assert t in kept and t not in weak and weak < kept
    assert all(S["strs"][b].size == l for a, l, b in weak)
    # on the records it changes nothing: with o_c == o the third record would be (c, b, len(c)), and no record overlaps the whole of its first string
    assert not any(l == S["strs"][a].size for a, l, b in every)


@pytest.mark.parametrize("both", [False, True])
def test_models_agree_on_the_designed_set_of_overlap(both):
    w, keep, kept, every = _agree(_index("overlap", both), L, both)
    assert 0 < len(kept) < len(every) and w["cnt"].max() >= 300


def test_models_agree_on_random_reads():
    S = _index("reads", True)
    assert len(S["strs"]) == 320
    w, keep, kept, every = _agree(S, 15, True)
    # one kept overlap per end for most reads, two for a few: about a sixth of the records
    assert _consequences(w, keep, True)[1] == 0                                          # reads of one length: no string ends inside another, the mirror rule is exact
    per_end = np.bincount(w["rec"][keep, 0], minlength=320)
    assert len(every) > 1500 and len(kept) < len(every) // 4 and per_end.max() <= 3 and int((per_end == 1).sum()) > 0.8 * int((per_end > 0).sum())
    _agree(S, 1, True)


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_rule_and_consequences_on_the_committed_indexes(name):
    fm = wm.Fm(km.read_plain(os.path.join(util.GOLDEN, name + ".bwt.gz")))
    strs = fm.retrieve(np.arange(int(fm.acc[1])))[1]
    for min_len in PLAIN[name]:
        w = om.walk(fm, min_len)
        keep = rm.reduce_records(w["rec"], w["lens"])
        assert keep.size == w["rec"].shape[0] and (min_len != PLAIN[name][2] or keep.size == 0)
        _consequences(w, keep, name in BOTH)
        if w["rec"].shape[0] <= 20000:
            assert np.array_equal(keep, _by_sets(w["rec"], w["lens"]))
        if sum(s.size ** 2 for s in strs) <= 10 ** 7:
            kept, every = rm.reduce_strings(strs, min_len)
            assert om.triples(w["rec"]) == every and _kept(w, keep) == kept


@pytest.mark.parametrize("both", [False, True])
def test_the_cap(both):
    """the rule is applied to the capped set: a record of a group that is left out is neither reduced nor a witness's first or third record.  (No mirror rule here:
    a record and its mirror image lie in groups of different sizes, and the cap may take a witness from one side only.)"""
    S = _index("reduce", both)
    w0, wc = om.walk(S["fm"], L), om.walk(S["fm"], L, CAP)
    assert wc["n_capped_groups"] > 0 and wc["rec"].shape[0] + wc["n_capped_hits"] == w0["rec"].shape[0]
    k0, kc = rm.reduce_records(w0["rec"], w0["lens"]), rm.reduce_records(wc["rec"], wc["lens"])
    assert np.array_equal(kc, _by_sets(wc["rec"], wc["lens"]))
    _consequences(wc, kc, False)
    all0, allc, kept0, keptc = om.triples(w0["rec"]), om.triples(wc["rec"]), _kept(w0, k0), _kept(wc, kc)
    assert allc < all0
    for name, c in rm.designed_cases().items():
        if "capped" not in c:
            continue
        t = (rm.row(c["a"], both), c["o"], rm.row(c["b"], both))
        assert t in all0 and t not in kept0, name                                        # reducible without the cap
        if c["capped"] == "kept":
            assert t in keptc and (t[0], 40, rm.row(c["c"], both)) not in allc, name     # its first record is in the group that is left out
        else:
            assert t not in allc and (rm.row(c["c"], both), 45, t[2]) not in allc, name   # the third record's group takes the record's own group with it
    assert {t for t in kept0 if t in allc} <= keptc                                       # the cap takes witnesses away, never adds one


def test_library_exports_the_reduction():
    lib = ctypes.CDLL(_build.LIB_GPU)
    assert hasattr(lib, "rb3gpu_overlap_reduced")
    from ropebwt3_amd import gpu
    assert "rb3gpu_overlap_reduced" in gpu.SYMBOLS and ctypes.sizeof(gpu.ReduceStats) == 6 * 8 + 9 * 8
    assert [k for k, _ in gpu.ReduceStats._fields_] == ["ms_total", "ms_count", "ms_who", "ms_emit", "ms_reduce", "ms_compact", "n_strings", "n_hits", "n_kept", "n_groups",
                                                        "n_capped_groups", "n_capped_hits", "n_emitters", "n_slices", "resident_bytes"]
    import inspect
    assert inspect.signature(gpu.Rb3Gpu.overlap).parameters["reduce"].default is False


def test_usage_lists_reduce():
    r = subprocess.run([CLI, "overlap"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and all(w in r.stderr for w in (b"--reduce", b"-l INT", b"-c INT", b"--pair", b"--gpu"))
