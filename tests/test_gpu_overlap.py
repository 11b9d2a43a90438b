"""`overlap` on the GPU against the model (tests/overlap_model.py): the designed set through the API on one strand and on both, with and without the early exit, the
counting walk in launches of a few strings and the emit stage in slices of a few records, the cap at its border, indexes of one and two strings, indexes that came
through a merge and through BRE records, the callback's return code, the refusals of the API, the command's bytes on FMD, FMR and BRE and its refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu
from ropebwt3_amd.gpu import OVERLAP_F, OVERLAP_REC, OverlapStats, Rb3GpuError
from tests import overlap_model as om
from tests import walk_model as wm

CLI = _build.BIN_CLI
L, CAP = om.MIN_LEN, om.CAP
LETTERS = np.frombuffer(b"$ACGTN", dtype=np.uint8)

_SET, _WALK = {}, {}


def _designed(both):
    """the designed set: its sequences, the strings of its rows, its BWT and its index as the model holds it -- computed once, shared, never changed"""
    if both not in _SET:
        seqs = om.designed(both=both)
        strs = om.rows_of(seqs, both)
        b = om.naive_bwt(strs)
        _SET[both] = dict(seqs=seqs, strs=strs, b=b, fm=wm.Fm(b), both=both)
    return _SET[both]


def _walk(S, min_len, max_hits=0, early=True):
    """the model's answer for the designed set: computed once per setting"""
    key = (S["both"], min_len, max_hits, early)
    if key not in _WALK:
        _WALK[key] = om.walk(S["fm"], min_len, max_hits, early)
    return _WALK[key]


def _check(h, w, min_len, max_hits=0, budget=None):
    """everything the API returns for the index on the handle against the model's walk w"""
    st = {}
    rec, lens = h.overlap(min_len, max_hits, stats=st, lengths=True)
    assert rec.dtype == OVERLAP_REC
    got = np.stack([rec["a"], rec["b"], rec["len"], rec["len_b"]], axis=1).astype(np.int64)
    assert got.shape == w["rec"].shape and np.array_equal(got, w["rec"])         # equal IN ORDER
    assert np.array_equal(lens, w["lens"])
    cnt = w["cnt"]
    want = dict(n_strings=cnt.size, n_steps_count=w["steps_count"], n_steps_emit=w["steps_emit"], n_early=w["n_early"], n_hits=int(cnt.sum()), n_groups=w["n_groups"],
                n_capped_groups=w["n_capped_groups"], n_capped_hits=w["n_capped_hits"], n_emitters=int((cnt > 0).sum()),
                n_slices=len(om.slices(cnt, budget if budget else 1 << 24)))
    assert {k: st[k] for k in want} == want
    assert np.array_equal(h.overlap(min_len, max_hits), rec)                     # without the lengths and the stats
    return st


# ---- 1. the designed set through the API ----

@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True])
def test_designed_set_through_the_api(both):
    S = _designed(both)
    assert S["b"].size > 2 * 8192
    longest = max(s.size for s in S["strs"])
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(S["b"])
        for early in (True, False):
            h.tune("ovl_early", int(early))
            for min_len in (L, 1):
                st = _check(h, _walk(S, min_len, 0, early), min_len)
                assert st["n_slices"] == 1 and st["n_hits"] > 0 and (st["n_early"] > 0) == early
            st = _check(h, _walk(S, longest + 1, 0, early), longest + 1)        # above every string: nothing to emit
            assert st["n_emitters"] == 0 and st["n_slices"] == 0 and st["n_hits"] == 0 and st["n_steps_emit"] == 0
            assert st["n_steps_count"] == (_walk(S, L, 0, True)["steps_count"] if early else S["b"].size)
        assert np.array_equal(_walk(S, L, 0, True)["rec"], _walk(S, L, 0, False)["rec"])
        assert np.array_equal(h.export_plain(), S["b"])                          # the index is not changed
    finally:
        h.close()


@pytest.mark.gpu
def test_no_callback_without_a_record():
    S = _designed(False)
    calls = []

    def cb(_ud, n, _recs):
        calls.append(int(n))
        return 0
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(S["b"])
        st = OverlapStats()
        assert h._lib.rb3gpu_overlap(h._h, 10 ** 6, 0, None, OVERLAP_F(cb), None, ctypes.byref(st)) == 0
        assert calls == [] and st.n_emitters == 0 and st.n_hits == 0 and st.n_slices == 0 and st.n_strings == len(S["strs"])
        assert h._lib.rb3gpu_overlap(h._h, 2 ** 40, 0, None, OVERLAP_F(cb), None, None) == 0 and calls == []
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("per", [1, 3])
def test_launches_of_a_few_strings(per):
    S = _designed(True)
    h = Rb3Gpu(verbose=1)
    try:
        h.tune("ovl_strings", per)
        h.from_plain(S["b"])
        _check(h, _walk(S, L), L)
        _check(h, _walk(S, L, CAP), L, CAP)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [1, 64])
def test_slices_of_a_few_records(budget):
    """a string with more records than the budget is a slice of its own: the one with 300 partners"""
    S = _designed(True)
    w = _walk(S, L)
    sl = om.slices(w["cnt"], budget)
    assert max(sl) == 300 and len(sl) > 10 and (budget > 1 or len(sl) == int((w["cnt"] > 0).sum()))
    h = Rb3Gpu(verbose=1)
    try:
        h.tune("ovl_slice", budget)
        h.from_plain(S["b"])
        st = _check(h, w, L, budget=budget)
        assert st["n_slices"] == len(sl)
        sizes = []

        def cb(_ud, n, _recs):
            sizes.append(int(n))
            return 0
        assert h._lib.rb3gpu_overlap(h._h, L, 0, None, OVERLAP_F(cb), None, None) == 0
        assert sizes == sl                                                       # the slices themselves
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True])
def test_the_cap_at_its_border(both):
    S = _designed(both)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(S["b"])
        for cap, groups, hits in ((CAP, 2, CAP + 1 + 300), (CAP + 1, 1, 300), (CAP - 1, 3, 2 * CAP + 1 + 300), (300, 0, 0), (299, 1, 300), (1, None, None)):
            w = _walk(S, L, cap)
            assert groups is None or (w["n_capped_groups"], w["n_capped_hits"]) == (groups, hits)
            st = _check(h, w, L, cap)
            assert st["n_capped_groups"] == w["n_capped_groups"] and st["n_hits"] + st["n_capped_hits"] == _walk(S, L)["rec"].shape[0]
        h.tune("ovl_early", 0)
        _check(h, _walk(S, L, CAP, False), L, CAP)
    finally:
        h.close()


# ---- 2. small indexes, and where the index comes from ----

A, C, G, T = 1, 2, 3, 4
SMALL = {
    "one": ([[A, C, G, A, C, G, A]], False),                      # overlaps itself at 4 and at 1
    "one_symbol": ([[G]], False),
    "two": ([[A, C, G, T, T], [T, T, G, C, A]], False),           # TT and T
    "two_both": ([[A, C, G, T, T], [G, T, C, C]], True),          # the reverse complement of the first, AACGT, ends as the second starts
    "equal": ([[A, C, A], [A, C, A]], False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_indexes(name):
    seqs, both = SMALL[name]
    strs = om.rows_of([np.array(s, dtype=np.uint8) for s in seqs], both)
    b = om.naive_bwt(strs)
    fm, bf = wm.Fm(b), om.Brute(strs)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(b)
        for early in (1, 0):
            h.tune("ovl_early", early)
            for min_len in (1, 2, 8):
                w = om.walk(fm, min_len, 0, bool(early))
                assert om.triples(w["rec"]) == bf.triples(min_len)
                _check(h, w, min_len)
        assert np.array_equal(h.export_plain(), b)
    finally:
        h.close()
    got = bf.triples(1)
    if name == "one":
        assert got == {(0, 4, 0), (0, 1, 0)}
    elif name == "one_symbol":
        assert got == set()
    elif name == "two":
        assert got == {(0, 2, 1), (0, 1, 1), (1, 1, 0)}
    elif name == "two_both":
        assert (1, 2, 2) in got and (3, 2, 0) in got
    elif name == "equal":
        assert got == {(a, 1, b_) for a in (0, 1) for b_ in (0, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["merge", "bre"])
def test_where_the_index_comes_from(source):
    S = _designed(True)
    h, h0 = Rb3Gpu(verbose=1), Rb3Gpu(verbose=1)
    try:
        if source == "merge":                                    # two batches through the merge path
            cut = len(S["seqs"]) // 2
            h.from_plain(om.naive_bwt(om.rows_of(S["seqs"][:cut], True)))
            h.merge_plain(om.naive_bwt(om.rows_of(S["seqs"][cut:], True)))
        else:
            h0.from_plain(S["b"])
            h.from_bre(h0.export_bre())
        assert np.array_equal(h.export_plain(), S["b"])
        _check(h, _walk(S, L), L)
        _check(h, _walk(S, L, CAP), L, CAP)
        assert np.array_equal(h.export_plain(), S["b"])
    finally:
        h.close()
        h0.close()


# ---- 3. the callback's return code and the refusals of the API ----

@pytest.mark.gpu
def test_the_callbacks_return_code_and_the_refusals():
    S = _designed(False)
    calls = []

    def cb(_ud, n, _recs):
        calls.append(int(n))
        return 7 if len(calls) == 2 else 0
    h, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.tune("ovl_slice", 64)
        h.from_plain(S["b"])
        lens = np.full(len(S["strs"]), -1, dtype=np.int64)
        assert h._lib.rb3gpu_overlap(h._h, L, 0, lens.ctypes.data, OVERLAP_F(cb), None, None) == 7
        assert calls == om.slices(_walk(S, L)["cnt"], 64)[:2]    # the call ends with the callback that refuses
        assert np.array_equal(lens, _walk(S, L)["lens"])         # filled before the first callback
        for args in ((0, 0), (-5, 0), (L, -1)):
            with pytest.raises(Rb3GpuError) as e:
                h.overlap(*args)
            assert e.value.code == -3
        assert h._lib.rb3gpu_overlap(h._h, L, 0, None, OVERLAP_F(), None, None) == -3
        _check(h, _walk(S, L), L, budget=64)                     # the handle still serves
        with pytest.raises(Rb3GpuError) as e:
            empty.overlap(L)
        assert e.value.code == -5
    finally:
        h.close()
        empty.close()


# ---- 4. the command ----

def _cli(args, env=None, cmd="overlap"):
    return subprocess.run([CLI, cmd] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


def _fasta(seqs):
    return "".join(">s%d\n%s\n" % (i, LETTERS[s].tobytes().decode()) for i, s in enumerate(seqs))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the designed set on both strands as FMD, FMR and BRE files, and on one strand as FMD, built by this command"""
    d = tmp_path_factory.mktemp("overlap")
    S = _designed(True)
    fa, fa1 = d / "set.fa", d / "fwd.fa"
    fa.write_text(_fasta(S["seqs"]))
    fa1.write_text(_fasta([s for s in _designed(False)["seqs"] if s.size]))       # (a FASTA record of no symbols is skipped by the reader)
    out = {}
    for ext, flag in (("fmd", "-d"), ("fmr", "-b"), ("bre", "-e")):
        out[ext] = str(d / ("set." + ext))
        _ok(_cli([flag, "-o", out[ext], str(fa)], cmd="build"))
    out["fwd"] = str(d / "fwd.fmd")
    _ok(_cli(["-d", "-R", "-o", out["fwd"], str(fa1)], cmd="build"))
    out["sorted"] = str(d / "sorted.fmr")
    _ok(_cli(["-b", "-r", "-o", out["sorted"], str(fa)], cmd="build"))
    junk = d / "junk.fmd"
    junk.write_bytes(b"this is not an index\n" * 7)
    out["junk"], out["nothing"] = str(junk), str(d / "nothing.fmd")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ext", ["fmd", "fmr", "bre"])
def test_cli_bytes(files, ext):
    S = _designed(True)
    w = _walk(S, L)
    assert _ok(_cli(["-l%d" % L, files[ext]])) == om.text(w["rec"], w["lens"])
    assert _ok(_cli(["-l", str(L), "--pair", files[ext]])) == om.text(w["rec"], w["lens"], pair=True)
    wc = _walk(S, L, CAP)
    assert _ok(_cli(["--pair", "-c", str(CAP), "-l", str(L), files[ext]])) == om.text(wc["rec"], wc["lens"], pair=True) != om.text(w["rec"], w["lens"], pair=True)
    if ext == "fmd":
        w31 = _walk(S, 31)
        assert _ok(_cli([files[ext]])) == om.text(w31["rec"], w31["lens"]) != b""                 # -l defaults to 31
        assert _ok(_cli(["-l", "1000", files[ext]])) == b""


@pytest.mark.gpu
def test_cli_on_one_strand(files):
    seqs = [s for s in _designed(False)["seqs"] if s.size]
    fm = wm.Fm(om.naive_bwt(seqs))
    w = om.walk(fm, L)
    assert _ok(_cli(["-l", str(L), files["fwd"]])) == om.text(w["rec"], w["lens"]) != b""


@pytest.mark.gpu
def test_cli_refusals_and_the_stats_line(files):
    for args in (["-l", "0", files["fmd"]], ["-l", "-3", files["fmd"]], ["-c", "-1", files["fmd"]], ["--pair", files["sorted"]], ["--pair", files["fwd"]],
                 [files["fmd"], "3"], [files["fmd"], files["fmd"]], [files["junk"]], [files["nothing"]]):
        r = _cli(args)
        err = r.stderr.decode().strip().splitlines()
        assert r.returncode == 1 and r.stdout == b"" and len(err) == 1 and err[0].startswith("ERROR"), (args, err)
    r = _cli([])
    assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr
    assert _ok(_cli(["-l", str(L), files["sorted"]])) != b""     # by rows a sorted index serves
    w = _walk(_designed(True), L)
    r = _cli(["--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3_VERBOSE="3"))
    _ok(r)
    line = [x for x in r.stderr.decode().splitlines() if "[M::main_overlap" in x]
    assert len(line) == 1 and all(x in line[0] for x in ("%d strings" % w["cnt"].size, "%d overlaps" % w["rec"].shape[0], "steps", "ended early", "count ", "emit "))
    r = _cli(["--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3_VERBOSE="2"))
    assert _ok(r) != b"" and b"main_overlap" not in r.stderr
