"""`overlap --reduce` on the GPU against the model (tests/reduce_model.py): the designed set and random reads through the API at three minimum lengths, every counter, the
same answers however the stages are cut into launches and slices, the cap, small indexes, indexes from a merge, from runs and from BRE records, the ceiling on the
resident records, the command's bytes and refusals, and the pipeline dedup | remove | overlap --reduce."""
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu
from ropebwt3_amd.gpu import OVERLAP_F, OVERLAP_REC, Rb3GpuError
from tests import dedup_model as dm
from tests import overlap_model as om
from tests import reduce_model as rm
from tests import walk_model as wm

CLI = _build.BIN_CLI
L, CAP = om.MIN_LEN, om.CAP
LETTERS = np.frombuffer(b"$ACGTN", dtype=np.uint8)

_SET, _WALK = {}, {}


def _index(name, both=True):
    """a set (the designed one, or the random reads): its sequences, the strings of its rows, its BWT and its index as the model holds it -- computed once, shared,
    never changed"""
    if (name, both) not in _SET:
        seqs = rm.designed_reduce(both=both) if name == "designed" else rm.read_set()
        strs = om.rows_of(seqs, both)
        b = om.naive_bwt(strs)
        _SET[(name, both)] = dict(seqs=seqs, strs=strs, b=b, fm=wm.Fm(b), key=(name, both))
    return _SET[(name, both)]


def _walk(S, min_len, max_hits=0):
    """the model's answer for a set: the walk's records and the keep mask of the rule, computed once per setting"""
    key = S["key"] + (min_len, max_hits)
    if key not in _WALK:
        w = om.walk(S["fm"], min_len, max_hits)
        _WALK[key] = dict(w, keep=rm.reduce_records(w["rec"], w["lens"]))
    return _WALK[key]


def _check(h, w, min_len, max_hits=0, budget=None):
    """everything the API returns for the index on the handle against the model"""
    st, st0 = {}, {}
    rec, lens = h.overlap(min_len, max_hits, stats=st, lengths=True, reduce=True)
    assert rec.dtype == OVERLAP_REC
    got = np.stack([rec["a"], rec["b"], rec["len"], rec["len_b"]], axis=1).astype(np.int64)
    want_rec = w["rec"][w["keep"]]
    assert got.shape == want_rec.shape and np.array_equal(got, want_rec)         # equal IN ORDER
    assert np.array_equal(lens, w["lens"])
    cnt = w["cnt"]
    kept = np.bincount(want_rec[:, 0], minlength=cnt.size)
    want = dict(n_strings=cnt.size, n_hits=int(cnt.sum()), n_kept=int(w["keep"].sum()), n_groups=w["n_groups"], n_capped_groups=w["n_capped_groups"],
                n_capped_hits=w["n_capped_hits"], n_emitters=int((cnt > 0).sum()), n_slices=len(om.slices(kept, budget if budget else 1 << 24)))
    assert {k: st[k] for k in want} == want
    assert np.array_equal(kept > 0, cnt > 0)                                     # the strings with kept records are the strings with records
    assert st["resident_bytes"] >= 28 * want["n_hits"] + 4 * cnt.size if want["n_hits"] else st["resident_bytes"] == 0
    all_rec = h.overlap(min_len, max_hits, stats=st0)                            # plain `overlap` on the same handle
    assert all(st0[k] == st[k] for k in ("n_hits", "n_groups", "n_capped_groups", "n_capped_hits", "n_emitters", "n_strings"))
    assert np.array_equal(all_rec[w["keep"]], rec)                               # a subsequence of its records
    return st


# ---- 1. the sets through the API ----

@pytest.mark.gpu
@pytest.mark.parametrize("name,both", [("designed", False), ("designed", True), ("reads", True)])
def test_sets_through_the_api(name, both):
    S = _index(name, both)
    longest = max(s.size for s in S["strs"])
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(S["b"])
        for min_len in (L, 1):
            st = _check(h, _walk(S, min_len), min_len)
            assert st["n_slices"] == 1 and 0 < st["n_kept"] < st["n_hits"]
        st = _check(h, _walk(S, longest + 1), longest + 1)                       # above every string: nothing to hold, nothing to deliver
        assert st["n_hits"] == 0 and st["n_kept"] == 0 and st["n_slices"] == 0 and st["n_emitters"] == 0
        assert np.array_equal(h.export_plain(), S["b"])                          # the index is not changed
    finally:
        h.close()
    if name == "designed":                                                       # what the set was designed to hold, as the GPU's answer has just been held to it
        w = _walk(S, L)
        assert w["cnt"].max() > 300
        kept = {(a, l, b) for a, b, l, _ in w["rec"][w["keep"]].tolist()}
        for case, c in rm.designed_cases().items():
            if c["strand"] and not both:
                continue
            bs, ks = (c["b"], c["kept"]) if case == "big" else ([c["b"]], [c["kept"]])
            for b, k in zip(bs, ks):
                assert ((rm.row(c["a"], both), c["o"], rm.row(b, both, c["strand"])) in kept) == k, case


@pytest.mark.gpu
@pytest.mark.parametrize("key,value", [("ovl_strings", 1), ("ovl_strings", 3), ("ovl_slice", 1), ("ovl_slice", 64), ("ovl_reduce_strings", 1), ("ovl_reduce_strings", 3),
                                       ("ovl_early", 0)])
def test_however_the_stages_are_cut(key, value):
    S = _index("designed")
    w, wc = _walk(S, L), _walk(S, L, CAP)
    budget = value if key == "ovl_slice" else None
    h = Rb3Gpu(verbose=1)
    try:
        h.tune(key, value)
        h.from_plain(S["b"])
        st = _check(h, w, L, budget=budget)
        _check(h, wc, L, CAP, budget=budget)
        if budget:                                                               # the slices themselves: by the KEPT records of consecutive strings
            kept = np.bincount(w["rec"][w["keep"], 0], minlength=w["cnt"].size)
            sl = om.slices(kept, budget)
            assert st["n_slices"] == len(sl) >= 10 and max(sl) == 201 and (budget > 1 or len(sl) == int((kept > 0).sum()))
            sizes = []

            def cb(_ud, n, _recs):
                sizes.append(int(n))
                return 0
            assert h._lib.rb3gpu_overlap_reduced(h._h, L, 0, None, OVERLAP_F(cb), None, None) == 0
            assert sizes == sl
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True])
def test_the_cap(both):
    S = _index("designed", both)
    w0, wc = _walk(S, L), _walk(S, L, CAP)
    assert wc["n_capped_groups"] > 0
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(S["b"])
        st = _check(h, wc, L, CAP)
        assert st["n_hits"] + st["n_capped_hits"] == w0["rec"].shape[0]
        _check(h, _walk(S, L, 1), L, 1)                                          # a cap of one: no string has two partners at one depth
    finally:
        h.close()
    kept0 = {(a, l, b) for a, b, l, _ in w0["rec"][w0["keep"]].tolist()}
    allc = {(a, l, b) for a, b, l, _ in wc["rec"].tolist()}
    keptc = {(a, l, b) for a, b, l, _ in wc["rec"][wc["keep"]].tolist()}
    for case, c in rm.designed_cases().items():
        if "capped" in c:
            t = (rm.row(c["a"], both), c["o"], rm.row(c["b"], both))
            assert t not in kept0 and ((t in keptc) if c["capped"] == "kept" else (t not in allc)), case


# ---- 2. small indexes, and where the index comes from ----

A, C, G, T = 1, 2, 3, 4
SMALL = {
    "one": ([[A, C, G, A, C, G, A, C, G, A]], False),             # overlaps itself at 7, 4 and 1: the first is kept, it is the witness of the others
    "one_symbol": ([[G]], False),
    "two": ([[A, C, G, T, T], [T, T, G, C, A]], False),           # TT and T
    "chain": ([[A, C, G, T], [C, G, T, A], [G, T, A, C]], False),  # 0 -> 1 -> 2 and 0 -> 2
    "equal": ([[A, C, A], [A, C, A]], False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_indexes(name):
    seqs, both = SMALL[name]
    strs = om.rows_of([np.array(s, dtype=np.uint8) for s in seqs], both)
    b = om.naive_bwt(strs)
    fm = wm.Fm(b)
    calls = []

    def cb(_ud, n, _recs):
        calls.append(int(n))
        return 0
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(b)
        for min_len in (1, 2, 8):
            w = om.walk(fm, min_len)
            w["keep"] = rm.reduce_records(w["rec"], w["lens"])
            kept, every = rm.reduce_strings(strs, min_len)
            assert {(a, l, b_) for a, b_, l, _ in w["rec"][w["keep"]].tolist()} == kept and om.triples(w["rec"]) == every
            _check(h, w, min_len)
            del calls[:]
            assert h._lib.rb3gpu_overlap_reduced(h._h, min_len, 0, None, OVERLAP_F(cb), None, None) == 0
            assert calls == ([len(kept)] if kept else [])                        # without a record the callback is never called
        assert np.array_equal(h.export_plain(), b)
    finally:
        h.close()
    kept = rm.reduce_strings(strs, 1)[0]
    if name == "one":
        assert kept == {(0, 7, 0)}
    elif name == "one_symbol":
        assert kept == set()
    elif name == "two":
        assert kept == {(0, 2, 1), (0, 1, 1), (1, 1, 0)}                         # (0, 1, 1) would need (1, 1, 4): TGCA does not start string 1
    elif name == "chain":
        assert (0, 3, 1) in kept and (1, 3, 2) in kept and (0, 2, 2) not in kept
    elif name == "equal":
        assert kept == {(a, 1, b_) for a in (0, 1) for b_ in (0, 1)}


def _runs(b):
    cut = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1], [True]]))
    return [(int(b[i]), int(j - i)) for i, j in zip(cut[:-1], cut[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["merge", "runs", "bre"])
def test_where_the_index_comes_from(source):
    S = _index("designed")
    h, h0 = Rb3Gpu(verbose=1), Rb3Gpu(verbose=1)
    try:
        if source == "merge":                                    # two batches through the merge path
            cut = len(S["seqs"]) // 2
            h.from_plain(om.naive_bwt(om.rows_of(S["seqs"][:cut], True)))
            h.merge_plain(om.naive_bwt(om.rows_of(S["seqs"][cut:], True)))
        elif source == "runs":
            h.from_runs(_runs(S["b"]))
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


# ---- 3. the ceiling on the resident records, the callback's return code and the refusals of the API ----

@pytest.mark.gpu
def test_the_resident_ceiling_and_the_refusals():
    S = _index("designed", False)
    w = _walk(S, L)
    n_hits = w["rec"].shape[0]
    calls = []

    def cb(_ud, n, _recs):
        calls.append(int(n))
        return 7 if len(calls) == 2 else 0
    h, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(S["b"])
        h.tune("ovl_resident", n_hits - 1)                       # one record too many
        assert h._lib.rb3gpu_overlap_reduced(h._h, L, 0, None, OVERLAP_F(cb), None, None) == -7 and calls == []
        with pytest.raises(Rb3GpuError) as e:
            h.overlap(L, reduce=True)
        assert e.value.code == -7
        assert h.overlap(L).shape[0] == n_hits                   # plain `overlap` knows no ceiling
        h.tune("ovl_resident", n_hits)                           # exactly enough
        _check(h, w, L)
        _check(h, _walk(S, L, CAP), L, CAP)                      # fewer records under the cap
        h.tune("ovl_resident", 0)
        h.tune("ovl_slice", 64)
        lens = np.full(len(S["strs"]), -1, dtype=np.int64)
        assert h._lib.rb3gpu_overlap_reduced(h._h, L, 0, lens.ctypes.data, OVERLAP_F(cb), None, None) == 7
        kept = np.bincount(w["rec"][w["keep"], 0], minlength=w["cnt"].size)
        assert calls == om.slices(kept, 64)[:2]                  # the call ends with the callback that refuses
        assert np.array_equal(lens, w["lens"])                   # filled before the first callback
        for args in ((0, 0), (-5, 0), (L, -1)):
            with pytest.raises(Rb3GpuError) as e:
                h.overlap(*args, reduce=True)
            assert e.value.code == -3
        assert h._lib.rb3gpu_overlap_reduced(h._h, L, 0, None, OVERLAP_F(), None, None) == -3
        _check(h, w, L, budget=64)                               # the handle still serves
        with pytest.raises(Rb3GpuError) as e:
            empty.overlap(L, reduce=True)
        assert e.value.code == -5
    finally:
        h.close()
        empty.close()


# ---- 4. the command ----

def _cli(args, env=None, cmd="overlap", data=None):
    return subprocess.run([CLI, cmd] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env, input=data)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


def _fasta(seqs):
    return "".join(">s%d\n%s\n" % (i, LETTERS[s].tobytes().decode()) for i, s in enumerate(seqs))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the designed set on both strands as FMD, FMR and BRE files, on one strand as FMD and sorted as FMR, built by this command"""
    d = tmp_path_factory.mktemp("reduce")
    fa = d / "set.fa"
    fa.write_text(_fasta(_index("designed")["seqs"]))
    out = {}
    for ext, flag in (("fmd", "-d"), ("fmr", "-b"), ("bre", "-e")):
        out[ext] = str(d / ("set." + ext))
        _ok(_cli([flag, "-o", out[ext], str(fa)], cmd="build"))
    out["fwd"] = str(d / "fwd.fmd")
    _ok(_cli(["-d", "-R", "-o", out["fwd"], str(fa)], cmd="build"))
    out["sorted"] = str(d / "sorted.fmr")
    _ok(_cli(["-b", "-r", "-o", out["sorted"], str(fa)], cmd="build"))
    junk = d / "junk.fmd"
    junk.write_bytes(b"this is not an index\n" * 7)
    out["junk"], out["nothing"] = str(junk), str(d / "nothing.fmd")
    return out


def _text(w, pair=False):
    return om.text(w["rec"][w["keep"]], w["lens"], pair=pair)


@pytest.mark.gpu
@pytest.mark.parametrize("ext", ["fmd", "fmr", "bre"])
def test_cli_bytes(files, ext):
    S = _index("designed")
    w, wc = _walk(S, L), _walk(S, L, CAP)
    assert _ok(_cli(["--reduce", "-l%d" % L, files[ext]])) == _text(w) != om.text(w["rec"], w["lens"])
    assert _ok(_cli(["-l", str(L), "--pair", "--reduce", files[ext]])) == _text(w, pair=True)
    assert _ok(_cli(["--pair", "--reduce", "-c", str(CAP), "-l", str(L), files[ext]])) == _text(wc, pair=True) != _text(w, pair=True)
    if ext == "fmd":
        assert _ok(_cli(["-l", str(L), files[ext]])) == om.text(w["rec"], w["lens"])              # without --reduce: every record, as before
        w31 = _walk(S, 31)
        assert _ok(_cli(["--reduce", files[ext]])) == _text(w31) != b""                           # -l defaults to 31
        assert _ok(_cli(["--reduce", "-l", "1000", files[ext]])) == b""


@pytest.mark.gpu
def test_cli_on_one_strand(files):
    w = _walk(_index("designed", False), L)
    assert _ok(_cli(["--reduce", "-l", str(L), files["fwd"]])) == _text(w) != b""


@pytest.mark.gpu
def test_cli_refusals_and_the_stats_line(files):
    for args in (["-l", "0", files["fmd"]], ["-l", "-3", files["fmd"]], ["-c", "-1", files["fmd"]], ["--pair", files["sorted"]], ["--pair", files["fwd"]],
                 [files["fmd"], "3"], [files["fmd"], files["fmd"]], [files["junk"]], [files["nothing"]]):
        r = _cli(["--reduce"] + args)
        err = r.stderr.decode().strip().splitlines()
        assert r.returncode == 1 and r.stdout == b"" and len(err) == 1 and err[0].startswith("ERROR"), (args, err)
    w = _walk(_index("designed"), L)
    n_hits = w["rec"].shape[0]
    # the ceiling on the resident records, through the environment's route to the tune keys
    r = _cli(["--reduce", "--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3GPU_OVL_RESIDENT=str(n_hits - 1)))
    err = r.stderr.decode().strip().splitlines()
    assert r.returncode == 1 and r.stdout == b"" and len(err) == 1 and err[0].startswith("ERROR") and "--reduce" in err[0] and "-l" in err[0] and "-c" in err[0], err
    assert _ok(_cli(["--reduce", "--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3GPU_OVL_RESIDENT=str(n_hits)))) == _text(w, pair=True)
    assert _ok(_cli(["--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3GPU_OVL_RESIDENT="1"))) == om.text(w["rec"], w["lens"], pair=True)
    assert _ok(_cli(["--reduce", "-l", str(L), files["sorted"]])) != b""         # by rows a sorted index serves
    r = _cli(["--reduce", "--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3_VERBOSE="3"))
    _ok(r)
    line = [x for x in r.stderr.decode().splitlines() if "[M::main_overlap" in x]
    assert len(line) == 1 and all(x in line[0] for x in ("%d strings" % w["cnt"].size, "%d overlaps" % n_hits, "%d kept" % int(w["keep"].sum()), "count ", "emit ",
                                                         "reduce ", "compact ", "resident"))
    r = _cli(["--reduce", "--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3_VERBOSE="2"))
    assert _ok(r) != b"" and b"main_overlap" not in r.stderr


@pytest.mark.gpu
def test_pipeline_from_dedup_and_remove(tmp_path):
    """dedup --pair X | remove --pair -d -f - X > U, then overlap --pair --reduce U: the model's answer for the sequences that stay.  The reads get copies, a reverse
    complement and reads that lie inside others, so that the first two steps have something to take out"""
    reads = rm.read_set()
    seqs = reads + [reads[3].copy(), reads[8][5:45].copy(), reads[20][0:30].copy(), reads[31][25:60].copy(), np.flip(5 - reads[40]).astype(np.uint8), reads[3].copy()]
    full, idx, u = tmp_path / "full.fa", tmp_path / "full.fmd", tmp_path / "u.fmd"
    full.write_text(_fasta(seqs))
    idx.write_bytes(_ok(_cli(["-d", str(full)], cmd="build")))
    kind = dm.kinds(dm.walk(wm.Fm(om.naive_bwt(om.rows_of(seqs, True))), True)[0], True)[0]
    stay = [s for i, s in enumerate(seqs) if kind[i] == dm.K]
    assert len(reads) - 20 < len(stay) <= len(seqs) - 6
    drop = _ok(_cli(["--pair", str(idx)], cmd="dedup"))
    assert drop == dm.drop_text(kind)
    u.write_bytes(_ok(_cli(["--pair", "-d", "-f", "-", str(idx)], cmd="remove", data=drop)))
    strs = om.rows_of(stay, True)
    w = om.walk(wm.Fm(om.naive_bwt(strs)), 15)
    w["keep"] = rm.reduce_records(w["rec"], w["lens"])
    kept, every = rm.reduce_strings(strs, 15)
    assert {(a, l, b) for a, b, l, _ in w["rec"][w["keep"]].tolist()} == kept and 0 < len(kept) < len(every) // 3
    assert _ok(_cli(["--pair", "--reduce", "-l", "15", str(u)])) == _text(w, pair=True)
    assert _ok(_cli(["--pair", "-l", "15", str(u)])) == om.text(w["rec"], w["lens"], pair=True)
