"""`dedup` on the GPU against the model (tests/dedup_model.py): the designed set through the API on one strand and on both, with and without the early exit, in
slices of a few strings, on indexes that came through a merge, from an FMR file this command built and through BRE records; tiny indexes at the borders of
the rule; one class of 3000 copies; the command's bytes, its refusals and the pipeline into `remove`."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, nt6_of
from tests import dedup_model as dm
from tests import kount_model as km
from tests import util
from tests import walk_model as wm

CLI = _build.BIN_CLI
G = lambda x: os.path.join(util.GOLDEN, x)    # noqa: E731

_SET = {}


def _designed(both):
    """the designed set: its sequences, the strings of its rows, its BWT and the model's answers -- computed once, shared, never changed"""
    if both not in _SET:
        seqs = dm.designed(both=both)
        strs = dm.rows_of(seqs, both)
        b = dm.naive_bwt(strs)
        fm = wm.Fm(b)
        _SET[both] = dict(seqs=seqs, strs=strs, b=b, early=dm.walk(fm, True), full=dm.walk(fm, False))
    return _SET[both]


def _check(h, S, pair, early=True, slices=None):
    """everything the API returns for the index of S on the handle against the model"""
    rec_w, steps_w, early_w = S["early" if early else "full"]
    for dup_only in (False, True):
        st = {}
        kind, keeper, rec = h.dedup(pair=pair, dup_only=dup_only, records=True, stats=st)
        want_kind, want_keeper = dm.kinds(rec_w, pair, dup_only)
        assert np.array_equal(np.stack([rec["occ"], rec["copies"], rec["cls"]], axis=1), rec_w), (pair, early, dup_only)
        assert np.array_equal(kind, want_kind) and np.array_equal(keeper, want_keeper), (pair, early, dup_only)
        assert st["n_steps"] == steps_w and st["n_early"] == early_w and st["n_strings"] == rec_w.shape[0]
        assert st["n_dup"] == int((want_kind == dm.D).sum()) and st["n_contained"] == int((want_kind == dm.C).sum())
        assert st["n_classes"] == np.unique(rec_w[rec_w[:, 1] > 1, 2]).size
        assert st["n_slices"] == (slices if slices is not None else 1)
        k2, p2 = h.dedup(pair=pair, dup_only=dup_only)           # without the records
        assert np.array_equal(k2, kind) and np.array_equal(p2, keeper)
    return kind


# ---- 1. the designed set through the API ----

@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True])
def test_designed_set_through_the_api(both):
    S = _designed(both)
    assert not both or S["b"].size > 2 * 8192
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(S["b"])
        fast = _check(h, S, both, early=True)
        h.tune("dedup_early", 0)
        full = _check(h, S, both, early=False)
        assert np.array_equal(fast, full) and S["full"][1] == S["b"].size > S["early"][1]
        if both:                                                 # an index of both strands read by rows: a string and its reverse complement are unrelated
            h.tune("dedup_early", 1)
            _check(h, S, False)
        assert np.array_equal(h.export_plain(), S["b"])          # the index is not changed
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slice_", [3, 1])
def test_slices(slice_):
    """classes span launches: the keeper table lives through all of them"""
    S = _designed(True)
    h = Rb3Gpu(verbose=1)
    try:
        h.tune("dedup_slice", slice_)
        h.from_plain(S["b"])
        _check(h, S, True, slices=-(-len(S["strs"]) // slice_))
    finally:
        h.close()


LETTERS = np.frombuffer(b"$ACGTN", dtype=np.uint8)


def _fasta(seqs):
    return "".join(">s%d\n%s\n" % (i, LETTERS[s].tobytes().decode()) for i, s in enumerate(seqs))


def _index_runs(path):
    """the runs of an FMD / FMR file as the host library reads them: [(symbol, length)]"""
    L = host.load_library()
    F = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64)
    L.rb3h_index_read_runs.restype = ctypes.c_int
    L.rb3h_index_read_runs.argtypes = [ctypes.c_char_p, F, ctypes.c_void_p]
    runs = []

    def emit(_d, c, l):
        runs.append((int(c), int(l)))
        return 0
    assert L.rb3h_index_read_runs(str(path).encode(), F(emit), None) >= 0
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["merge", "fmr", "bre"])
def test_where_the_index_comes_from(source, tmp_path):
    S = _designed(True)
    h, h0 = Rb3Gpu(verbose=1), Rb3Gpu(verbose=1)
    try:
        if source == "merge":                                    # two batches through the merge path
            cut = len(S["seqs"]) // 2
            h.from_plain(dm.naive_bwt(dm.rows_of(S["seqs"][:cut], True)))
            h.merge_plain(dm.naive_bwt(dm.rows_of(S["seqs"][cut:], True)))
        else:
            h0.from_plain(S["b"])
            if source == "fmr":                                  # an FMR file of the designed set built by this command, read through the host's decoder
                fa, fmr = tmp_path / "set.fa", tmp_path / "set.fmr"
                fa.write_text(_fasta(S["seqs"]))
                r = subprocess.run([CLI, "build", "-b", "-o", str(fmr), str(fa)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
                assert r.returncode == 0 and fmr.read_bytes()[:4] == b"RB\2\0", r.stderr.decode(errors="replace")[-2000:]
                h.from_runs(_index_runs(fmr))
            else:
                h.from_bre(h0.export_bre())
        assert np.array_equal(h.export_plain(), S["b"])
        _check(h, S, True)
    finally:
        h.close()
        h0.close()
    if source == "fmr":                                          # ... and the command on that file: the header, the order byte and the decoder in front of dedup
        rec = S["early"][0]
        for pair in (False, True):
            for dup_only in (False, True):
                kind, keeper = dm.kinds(rec, pair, dup_only)
                flags = (["--pair"] if pair else []) + (["--dup-only"] if dup_only else [])
                r = subprocess.run([CLI, "dedup"] + flags + [str(fmr)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
                assert r.returncode == 0 and r.stdout == dm.drop_text(kind), (flags, r.stderr.decode(errors="replace")[-2000:])
                r = subprocess.run([CLI, "dedup", "--table"] + flags + [str(fmr)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
                assert r.returncode == 0 and r.stdout == dm.table_text(kind, keeper, rec, pair), flags


# ---- 2. borders ----

A, Cc, Gg, T = 1, 2, 3, 4
BORDERS = {
    "only_empty": ([[], [], []], False),
    "single": ([[A, Cc, Gg, Gg, T, A]], False),
    "first_symbol": ([[A, Cc, Gg, T, T], [Cc, Cc, Gg, T, T]], False),
    "last_symbol": ([[A, Cc, Gg, T, T], [A, Cc, Gg, T, A]], False),
    "exit_at_the_sentinel": ([[A, Cc, Gg, T], [T, Cc, Gg, T]], False),       # CGT twice, ACGT once: the interval is one row only with the string's first symbol
    "chain": ([[A], [A, A], [A, A, A]], False),
    "palindrome": ([[A, Cc, Gg, T]], True),
    "palindrome_twice": ([[A, A, T, T], [Gg], [A, A, T, T]], True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BORDERS))
def test_borders(name):
    seqs, both = BORDERS[name]
    strs = dm.rows_of([np.array(s, dtype=np.uint8) for s in seqs], both)
    b = dm.naive_bwt(strs)
    fm = wm.Fm(b)
    bf = dm.Brute(strs)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(b)
        for early in (1, 0):
            h.tune("dedup_early", early)
            S = {"early": dm.walk(fm, True), "full": dm.walk(fm, False)}
            kind = _check(h, S, both, early=bool(early))
            assert np.array_equal(kind, bf.kinds(both, True)[0])
            assert np.array_equal(h.dedup(pair=both)[0], bf.kinds(both, False)[0])
    finally:
        h.close()
    full, fast = dm.walk(fm, False)[0], dm.walk(fm, True)
    assert np.array_equal(full[:, 0], bf.occ) and np.array_equal(full[:, 1], bf.copies)
    kind = dm.kinds(full, both)[0].tobytes()
    if name == "only_empty":
        assert kind == b"KDD" and (full[:, 0] == 3).all() and (full[:, 1] == 3).all()
    elif name == "chain":
        assert kind == b"CCK" and full[:, 0].tolist() == [6, 3, 1]
    elif name == "exit_at_the_sentinel":
        assert kind == b"KK" and fast[2] == 2 and fast[1] == 2 * 4     # both walks end early, on the step of their first symbol
    elif name in ("first_symbol", "last_symbol", "single", "palindrome"):
        assert set(kind) == {dm.K}
    elif name == "palindrome_twice":
        assert kind == b"KKD"


# ---- 3. one wide class ----

@pytest.mark.gpu
def test_copies3000():
    lines = [x for x in gzip.open(G("copies3000.txt.gz")).read().split(b"\n") if x]
    strs = dm.rows_of([nt6_of(x.decode()) for x in lines], True)
    bf = dm.Brute(strs)
    want_kind, want_keeper = bf.kinds(pair=True)
    assert want_kind.tobytes() == b"K" + b"D" * 2999 and (want_keeper == 0).all()
    h = Rb3Gpu(verbose=1)
    try:
        h.from_fmd_file(G("copies3000.fmd"))
        st = {}
        kind, keeper, rec = h.dedup(pair=True, records=True, stats=st)
        assert np.array_equal(kind, want_kind) and np.array_equal(keeper, want_keeper)
        assert np.array_equal(rec["occ"], bf.occ) and np.array_equal(rec["copies"], bf.copies) and np.unique(rec["cls"]).size == 2
        assert st["n_classes"] == 2 and st["n_dup"] == 2999 and st["n_early"] == 0
        assert st["n_steps"] == sum(s.size + 1 for s in strs)    # no walk ends early: every row of the index is read once
    finally:
        h.close()
    r = subprocess.run([CLI, "dedup", "--pair", G("copies3000.fmd")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout == dm.drop_text(want_kind)


# ---- 4. the command ----

def _cli(args, env=None, cmd="dedup", data=None):
    return subprocess.run([CLI, cmd] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env, input=data)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


_MODEL = {}


def _model(name):
    if name not in _MODEL:
        _MODEL[name] = dm.walk(wm.Fm(km.read_plain(G(name + ".bwt.gz"))), True)[0]
    return _MODEL[name]


@pytest.mark.gpu
@pytest.mark.parametrize("idx", ["edge_dups.fmd", "reads_fq.fmd", "edge_dups.bre"])
def test_cli_bytes(idx):
    rec = _model(os.path.splitext(idx)[0])
    for pair in (False, True):
        for dup_only in (False, True):
            kind, keeper = dm.kinds(rec, pair, dup_only)
            flags = (["--pair"] if pair else []) + (["--dup-only"] if dup_only else [])
            assert _ok(_cli(flags + [G(idx)])) == dm.drop_text(kind), flags
            assert _ok(_cli(flags + ["--table", G(idx)])) == dm.table_text(kind, keeper, rec, pair), flags
    if idx.startswith("edge_dups"):
        assert dm.drop_text(dm.kinds(rec, False, True)[0]) != dm.drop_text(dm.kinds(rec, False, False)[0])  # --dup-only changes the answer here


@pytest.mark.gpu
def test_cli_refusals_and_the_stats_line(tmp_path):
    junk = tmp_path / "junk.fmd"
    junk.write_bytes(b"this is not an index\n" * 7)
    sorted_idx = tmp_path / "sorted.fmr"
    sorted_idx.write_bytes(_ok(_cli(["-b", "-r", "-L", G("edge_dups.txt")], cmd="build")))
    assert sorted_idx.read_bytes()[:3] == b"RB\2" and sorted_idx.read_bytes()[3] in (1, 2)
    for args in (["--pair", str(sorted_idx)], ["--pair", G("reads_fwd.fmd")], ["--pair", G("k2_fwd.fmd")], [G("edge_dups.fmd"), "3"], [G("edge_dups.fmd"), G("edge_dups.fmd")],
                 [str(junk)], [str(tmp_path / "nothing.fmd")]):
        r = _cli(args)
        err = r.stderr.decode().strip().splitlines()
        assert r.returncode == 1 and r.stdout == b"" and len(err) == 1 and err[0].startswith("ERROR"), (args, err)
    _ok(_cli([str(sorted_idx)]))                                # by rows a sorted index serves
    r = _cli(["--pair", G("edge_dups.fmd")], env=dict(os.environ, RB3_VERBOSE="3"))
    _ok(r)
    line = [x for x in r.stderr.decode().splitlines() if "[M::main_dedup" in x]
    assert len(line) == 1 and all(w in line[0] for w in ("12 strings", "duplicates", "contained", "steps", "ended early", "walk "))
    r = _cli(["--pair", G("edge_dups.fmd")], env=dict(os.environ, RB3_VERBOSE="2"))
    assert _ok(r) != b"" and b"main_dedup" not in r.stderr


@pytest.mark.gpu
def test_pipeline_into_remove(tmp_path):
    """dedup --pair X | remove --pair -d -f - X is build -d of the sequences that stay, and dedup finds nothing more in it"""
    S = _designed(True)
    fa = _fasta
    full, rest, idx = tmp_path / "full.fa", tmp_path / "rest.fa", tmp_path / "full.fmd"
    full.write_text(fa(S["seqs"]))
    idx.write_bytes(_ok(_cli(["-d", str(full)], cmd="build")))
    kind = dm.kinds(S["early"][0], True)[0]
    drop = _ok(_cli(["--pair", str(idx)]))
    assert drop == dm.drop_text(kind) and 16 <= len(drop.splitlines()) < len(S["seqs"])
    got = _ok(_cli(["--pair", "-d", "-f", "-", str(idx)], cmd="remove", data=drop))
    rest.write_text(fa([s for u, s in enumerate(S["seqs"]) if kind[u] == dm.K]))
    assert got == _ok(_cli(["-d", str(rest)], cmd="build"))
    if os.path.exists(util.REF_BIN):
        assert got == _ok(subprocess.run([util.REF_BIN, "build", "-d", str(rest)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300))
    out = tmp_path / "dedup.fmd"
    out.write_bytes(got)
    assert _ok(_cli(["--pair", str(out)])) == b""


# ---- 5. pair on an index that is not of both strands ----

@pytest.mark.gpu
def test_pair_on_an_asymmetric_index():
    rng = np.random.default_rng(5)
    strs = [util.random_genome(rng, int(rng.integers(5, 60))) for _ in range(10)]
    strs[7] = strs[2].copy()
    b = dm.naive_bwt(strs)
    rec = dm.walk(wm.Fm(b), True)[0]
    with pytest.raises(ValueError):
        dm.kinds(rec, pair=True)
    h, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(b)
        with pytest.raises(Rb3GpuError) as e:
            h.dedup(pair=True)
        assert e.value.code == -3
        kind, keeper = h.dedup()                                 # the handle still serves
        assert np.array_equal(kind, dm.kinds(rec)[0]) and np.array_equal(keeper, dm.kinds(rec)[1]) and kind[7] == dm.D and keeper[7] == 2
        assert np.array_equal(h.export_plain(), b)
        h.from_plain(dm.naive_bwt(strs[:9]))                     # an odd number of strings
        with pytest.raises(Rb3GpuError) as e:
            h.dedup(pair=True)
        assert e.value.code == -3
        with pytest.raises(Rb3GpuError) as e:
            empty.dedup()
        assert e.value.code == -5
    finally:
        h.close()
        empty.close()
