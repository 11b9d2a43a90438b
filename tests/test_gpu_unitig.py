"""`unitig` on the GPU against the model (tests/unitig_model.py): every set through the API with and without `pair` -- unitigs, members, symbols and links in order, every
counter --, the same answers however the stages are cut, indexes from a merge, from runs and from BRE records, the cap, the refusals of an asymmetric graph and of the
resident ceiling, the command's bytes and refusals, and the pipeline dedup | remove | unitig."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu
from ropebwt3_amd.gpu import UNITIG_F, UNITIG_LINK_F, UNITIG_LINK, UNITIG_MEMBER, UNITIG_REC, Rb3GpuError, UnitigStats
from tests import dedup_model as dm
from tests import overlap_model as om
from tests import reduce_model as rm
from tests import unitig_model as um
from tests import walk_model as wm

CLI = _build.BIN_CLI
L, CAP = um.L, om.CAP
LETTERS = np.frombuffer(b"$ACGTN", dtype=np.uint8)

_SETS, _SET, _ANS = um.SETS(), {}, {}


def _index(name):
    """a set: its sequences, the strings of its rows, its BWT and its index as the model holds it -- computed once, shared, never changed"""
    if name not in _SET:
        seqs, both = _SETS[name]
        strs = om.rows_of(seqs, both)
        b = om.naive_bwt(strs)
        _SET[name] = dict(seqs=seqs, strs=strs, both=both, b=b, fm=wm.Fm(b), key=name)
    return _SET[name]


def _model(S, pair, min_len=L, max_hits=0):
    """the model's answer for a set: the walk, the rule on its records, then the unitigs by both restatements -- computed once per setting"""
    key = (S["key"], pair, min_len, max_hits)
    if key not in _ANS:
        w = om.walk(S["fm"], min_len, max_hits)
        K = w["rec"][rm.reduce_records(w["rec"], w["lens"])]
        a, j = um.sequential(K, w["lens"], pair), um.jumping(K, w["lens"], pair)
        assert a["refused"] == j["refused"] and all(np.array_equal(a[k], j[k]) for k in a if k in j)
        a.update(n_rounds=j["n_rounds"], n_hits=int(w["rec"].shape[0]), seqs=None if a["refused"] else um.spell(a, S["strs"]))
        _ANS[key] = a
    return _ANS[key]


def _check(h, a, pair, min_len=L, max_hits=0, budget=None):
    """everything the API returns for the index on the handle against the model"""
    st = {}
    utg, mem, seqs, links = h.unitigs(min_len, max_hits, pair=pair, links=True, stats=st)
    assert utg.dtype == UNITIG_REC and mem.dtype == UNITIG_MEMBER and links.dtype == UNITIG_LINK
    got_u = np.stack([utg[k] for k in ("head", "tail", "members", "circ", "len")], axis=1).astype(np.int64)
    got_m = np.stack([mem[k] for k in ("row", "o_in", "off")], axis=1).astype(np.int64)
    got_l = np.stack([links[k] for k in ("from", "from_rev", "to", "to_rev", "len")], axis=1).astype(np.int64)
    assert np.array_equal(got_u, a["utg"]) and np.array_equal(got_m, a["mem"]) and np.array_equal(got_l, a["links"])      # equal IN ORDER
    assert len(seqs) == len(a["seqs"]) and all(np.array_equal(x, y) for x, y in zip(seqs, a["seqs"]))
    want = {k: a[k] for k in ("n_strings", "n_kept", "n_simple", "n_unitigs", "n_members", "n_symbols", "n_cycles", "n_asym", "n_links", "max_members", "n_rounds")}
    want.update(n_steps_emit=a["n_symbols"], n_slices=len(om.slices(a["utg"][:, 4], budget if budget else 1 << 26)))   # one LF step per symbol of the output, exactly
    assert {k: st[k] for k in want} == want
    lg = lambda x: max(0, math.ceil(math.log2(max(x, 1))))    # noqa: E731
    assert st["n_rounds"] <= lg(a["max_members"]) + lg(a["n_strings"]) + 1       # DESIGN.md 7s (with pair the chains that are not output are mirror images: as long)
    if a["n_cycles"] == 0:
        assert st["n_rounds"] <= lg(a["max_members"]) + 1
    assert st["resident_bytes"] >= 100 * a["n_strings"] + 28 * a["n_hits"]
    return st


# ---- 1. the sets through the API ----

CASES = [(name, pair) for name, (_, both) in _SETS.items() for pair in ((False, True) if both else (False,)) if not (pair and name in um.ASYM)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,pair", CASES)
def test_sets_through_the_api(name, pair):
    S = _index(name)
    a = _model(S, pair)
    longest = max(s.size for s in S["strs"])
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(S["b"])
        st = _check(h, a, pair)
        assert st["n_slices"] == 1
        _check(h, _model(S, pair, min_len=longest + 1), pair, min_len=longest + 1)    # no overlap at all: every string is a unitig of its own
        assert np.array_equal(h.export_plain(), S["b"])                          # the index is not changed
    finally:
        h.close()
    one = _model(S, pair, min_len=longest + 1)
    assert one["n_kept"] == 0 and one["n_links"] == 0 and one["max_members"] == 1 and one["n_unitigs"] == (len(S["seqs"]) if pair or not S["both"] else 2 * len(S["seqs"]))


@pytest.mark.gpu
@pytest.mark.parametrize("key,value", [("utg_slice", 1), ("utg_slice", 64), ("utg_strings", 1), ("utg_strings", 3), ("ovl_strings", 1), ("ovl_strings", 3),
                                       ("ovl_reduce_strings", 1), ("ovl_reduce_strings", 3)])
def test_however_the_stages_are_cut(key, value):
    budget = value if key == "utg_slice" else None
    for name, pair in (("designed1", False), ("designed2", True), ("designed2", False)):
        S = _index(name)
        a = _model(S, pair)
        h = Rb3Gpu(verbose=1)
        try:
            h.tune(key, value)
            h.from_plain(S["b"])
            st = _check(h, a, pair, budget=budget)
            if budget:                                                           # the slices themselves: consecutive unitigs by their lengths
                sl = om.slices(a["utg"][:, 4], budget)
                assert st["n_slices"] == len(sl) and (budget > 1 or len(sl) == a["n_unitigs"])
                sizes = []

                def cb(_ud, u0, n, _u, _m, off, _s):
                    sizes.append((int(u0), int(np.frombuffer(ctypes.string_at(off, (int(n) + 1) * 8), dtype=np.int64)[int(n)])))
                    return 0
                assert h._lib.rb3gpu_unitigs(h._h, L, 0, int(pair), UNITIG_F(cb), None, UNITIG_LINK_F(), None) == 0
                assert [s for _, s in sizes] == sl and [u for u, _ in sizes] == [0] + np.cumsum([len(x) for x in _cut(a["utg"][:, 4], budget)])[:-1].tolist()
        finally:
            h.close()


def _cut(lens, budget):
    out, tot = [[]], 0
    for x in lens.tolist():
        if out[-1] and tot + x > budget:
            out.append([])
            tot = 0
        out[-1].append(x)
        tot += x
    return out


def _runs(b):
    cut = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1], [True]]))
    return [(int(b[i]), int(j - i)) for i, j in zip(cut[:-1], cut[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["merge", "runs", "bre"])
def test_where_the_index_comes_from(source):
    S = _index("designed2")
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
        _check(h, _model(S, True), True)
        _check(h, _model(S, False), False)
        assert np.array_equal(h.export_plain(), S["b"])
    finally:
        h.close()
        h0.close()


@pytest.mark.gpu
def test_the_cap():
    S = _index("reduce1")
    a0, ac = _model(S, False), _model(S, False, max_hits=CAP)
    assert ac["n_hits"] < a0["n_hits"] and not np.array_equal(a0["utg"], ac["utg"])
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(S["b"])
        _check(h, ac, False, max_hits=CAP)
        _check(h, _model(S, False, max_hits=1), False, max_hits=1)
    finally:
        h.close()


# ---- 2. the refusals of the API ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(um.ASYM))
def test_an_asymmetric_graph_is_refused(name):
    S = _index(name)
    a = _model(S, True)
    assert a["refused"] and a["n_asym"] == um.ASYM[name]
    calls = []

    def cb(*_args):
        calls.append(1)
        return 0
    h = Rb3Gpu(verbose=0)
    try:
        h.from_plain(S["b"])
        st = UnitigStats()
        assert h._lib.rb3gpu_unitigs(h._h, L, 0, 1, UNITIG_F(cb), None, UNITIG_LINK_F(cb), ctypes.byref(st)) == -7 and calls == []
        assert (st.n_asym, st.n_kept, st.n_simple, st.n_unitigs) == (a["n_asym"], a["n_kept"], a["n_simple"], 0)
        got = {}
        with pytest.raises(Rb3GpuError) as e:
            h.unitigs(L, pair=True, stats=got)
        assert e.value.code == -7 and got["n_asym"] == a["n_asym"]
        _check(h, _model(S, False), False)                                       # without pair no symmetry is asked for, and the handle still serves
    finally:
        h.close()


@pytest.mark.gpu
def test_the_resident_ceiling_and_the_refusals():
    S = _index("designed1")
    a = _model(S, False)
    calls = []

    def cb(_ud, _u0, n, *_rest):
        calls.append(int(n))
        return 7 if len(calls) == 2 else 0
    h, empty, odd = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(S["b"])
        h.tune("ovl_resident", a["n_hits"] - 1)                  # one record too many
        st = UnitigStats()
        assert h._lib.rb3gpu_unitigs(h._h, L, 0, 0, UNITIG_F(cb), None, UNITIG_LINK_F(), ctypes.byref(st)) == -7 and calls == [] and st.n_asym == 0
        h.tune("ovl_resident", a["n_hits"])                      # exactly enough
        _check(h, a, False)
        h.tune("ovl_resident", 0)
        h.tune("utg_slice", 64)
        assert h._lib.rb3gpu_unitigs(h._h, L, 0, 0, UNITIG_F(cb), None, UNITIG_LINK_F(), None) == 7
        assert calls == [len(x) for x in _cut(a["utg"][:, 4], 64)[:2]]           # the call ends with the callback that refuses
        for args in ((0, 0), (-5, 0), (L, -1)):
            with pytest.raises(Rb3GpuError) as e:
                h.unitigs(*args)
            assert e.value.code == -3
        assert h._lib.rb3gpu_unitigs(h._h, L, 0, 0, UNITIG_F(), None, UNITIG_LINK_F(), None) == -3
        _check(h, a, False, budget=64)                           # the handle still serves
        with pytest.raises(Rb3GpuError) as e:
            empty.unitigs(L)
        assert e.value.code == -5
        odd.from_plain(om.naive_bwt([np.array([1, 2, 3], dtype=np.uint8)]))
        with pytest.raises(Rb3GpuError) as e:
            odd.unitigs(1, pair=True)                            # one string is not both strands of anything
        assert e.value.code == -3
    finally:
        h.close()
        empty.close()
        odd.close()


# ---- 3. the command ----

def _cli(args, env=None, cmd="unitig", data=None):
    return subprocess.run([CLI, cmd] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env, input=data)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


def _fasta(seqs):
    return "".join(">s%d\n%s\n" % (i, LETTERS[s].tobytes().decode()) for i, s in enumerate(seqs))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """designed2 on both strands as FMD, FMR and BRE files, designed1 on one strand as FMD, the asymmetric sets, and a sorted index, all built by this command"""
    d = tmp_path_factory.mktemp("unitig")
    out = {}
    for name in ("designed2", "designed1", "contained2", "reduce2"):
        fa = d / (name + ".fa")
        fa.write_text(_fasta(_SETS[name][0]))
        out[name + ".fa"] = str(fa)
    for ext, flag in (("fmd", "-d"), ("fmr", "-b"), ("bre", "-e")):
        out[ext] = str(d / ("set." + ext))
        _ok(_cli([flag, "-o", out[ext], out["designed2.fa"]], cmd="build"))
    out["fwd"] = str(d / "fwd.fmd")
    _ok(_cli(["-d", "-R", "-o", out["fwd"], out["designed1.fa"]], cmd="build"))
    out["sorted"] = str(d / "sorted.fmr")
    _ok(_cli(["-b", "-r", "-o", out["sorted"], out["designed2.fa"]], cmd="build"))
    for name in ("contained2", "reduce2"):
        out[name] = str(d / (name + ".fmd"))
        _ok(_cli(["-d", "-o", out[name], out[name + ".fa"]], cmd="build"))
    junk = d / "junk.fmd"
    junk.write_bytes(b"this is not an index\n" * 7)
    out["junk"], out["nothing"] = str(junk), str(d / "nothing.fmd")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ext", ["fmd", "fmr", "bre"])
def test_cli_bytes(files, ext):
    S = _index("designed2")
    ap, a = _model(S, True), _model(S, False)
    assert _ok(_cli(["--pair", "-l%d" % L, files[ext]])) == um.text(ap, ap["seqs"]) != b""
    assert _ok(_cli(["-l", str(L), "--pair", "--gfa", files[ext]])) == um.gfa(ap, ap["seqs"])
    assert _ok(_cli(["-l", str(L), "--pair", "--table", files[ext]])) == um.table(ap, pair=True)
    assert _ok(_cli(["-l", str(L), files[ext]])) == um.text(a, a["seqs"]) != um.text(ap, ap["seqs"])
    if ext == "fmd":
        assert _ok(_cli(["-l", str(L), "--gfa", files[ext]])) == um.gfa(a, a["seqs"])
        assert _ok(_cli(["-l", str(L), "--table", files[ext]])) == um.table(a)
        a31 = _model(S, True, min_len=31)
        assert _ok(_cli(["--pair", files[ext]])) == um.text(a31, a31["seqs"])                     # -l defaults to 31
        g = um.gfa(ap, ap["seqs"]).splitlines()
        assert g[0] == b"H\tVN:Z:1.0" and sum(x.startswith(b"S\t") for x in g) == ap["n_unitigs"] and sum(x.startswith(b"L\t") for x in g) == ap["n_links"] + ap["n_cycles"]
        assert b"\tCL:i:40\n" in um.text(ap, ap["seqs"]) and b"\tCL:i:30\n" in um.text(ap, ap["seqs"])


@pytest.mark.gpu
def test_cli_on_one_strand(files):
    a = _model(_index("designed1"), False)
    assert _ok(_cli(["-l", str(L), files["fwd"]])) == um.text(a, a["seqs"]) != b""
    assert _ok(_cli(["--gfa", "-l", str(L), files["fwd"]])) == um.gfa(a, a["seqs"])


@pytest.mark.gpu
def test_cli_refusals_and_the_stats_line(files):
    for args in (["-l", "0", files["fmd"]], ["-l", "-3", files["fmd"]], ["-c", "-1", files["fmd"]], ["--gfa", "--table", files["fmd"]], ["--pair", files["sorted"]],
                 ["--pair", files["fwd"]], [files["fmd"], "3"], [files["junk"]], [files["nothing"]], ["--reduce", files["fmd"]], ["-x", files["fmd"]],
                 ["--pair", "-l", str(L), files["contained2"]], ["--pair", "-l", str(L), files["reduce2"]], ["--pair", "--gfa", "-l", str(L), files["reduce2"]]):
        r = _cli(args)
        err = r.stderr.decode().strip().splitlines()
        assert r.returncode == 1 and r.stdout == b"" and len(err) == 1, (args, err)
        assert err[0].startswith("ERROR") or "option" in err[0], (args, err)
    for args in (["--pair", files["sorted"]], ["--pair", files["fwd"]]):         # what `overlap --pair` refuses, with the same message
        assert _cli(args).stderr == _cli(args, cmd="overlap").stderr
    err = _cli(["--pair", "-l", str(L), files["reduce2"]]).stderr.decode()
    assert all(x in err for x in ("dedup --pair", "remove --pair", "-c", "without --pair")) and " 2 overlaps" in err
    assert _ok(_cli(["-l", str(L), files["reduce2"]])) != b""                    # without --pair it serves
    S = _index("designed2")
    a = _model(S, True)
    # the ceiling on the resident records, through the environment's route to the tune keys: the two messages of overlap --reduce
    r = _cli(["--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3GPU_OVL_RESIDENT=str(a["n_hits"] - 1)))
    r0 = _cli(["--pair", "--reduce", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3GPU_OVL_RESIDENT=str(a["n_hits"] - 1)), cmd="overlap")
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == r0.stderr and r.stderr.startswith(b"ERROR") and r.stderr.count(b"\n") == 1
    assert _ok(_cli(["--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3GPU_OVL_RESIDENT=str(a["n_hits"])))) == um.text(a, a["seqs"])
    r = _cli(["--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3_VERBOSE="3"))
    _ok(r)
    line = [x for x in r.stderr.decode().splitlines() if "[M::main_unitig" in x]
    assert len(line) == 1 and all(x in line[0] for x in ("%d strings" % a["n_strings"], "%d kept" % a["n_kept"], "%d simple" % a["n_simple"], "%d unitigs" % a["n_unitigs"],
                                                         "%d symbols" % a["n_symbols"], "%d links" % a["n_links"], "%d rounds" % a["n_rounds"], "reduce ", "graph ", "rank ",
                                                         "emit ", "resident"))
    r = _cli(["--pair", "-l", str(L), files["fmd"]], env=dict(os.environ, RB3_VERBOSE="2"))
    assert _ok(r) != b"" and b"main_unitig" not in r.stderr


@pytest.mark.gpu
def test_pipeline_from_dedup_and_remove(tmp_path):
    """dedup --pair X | remove --pair -d -f - X > U, then unitig --pair --gfa U: the model's answer for the sequences that stay.  The reads get copies, a reverse
    complement and reads that lie inside others, so that the first two steps have something to take out -- and without them the graph is refused"""
    reads = rm.read_set()
    seqs = reads + [reads[3].copy(), reads[8][5:45].copy(), reads[20][0:30].copy(), reads[31][25:60].copy(), np.flip(5 - reads[40]).astype(np.uint8), reads[3].copy()]
    full, idx, u = tmp_path / "full.fa", tmp_path / "full.fmd", tmp_path / "u.fmd"
    full.write_text(_fasta(seqs))
    idx.write_bytes(_ok(_cli(["-d", str(full)], cmd="build")))
    kind = dm.kinds(dm.walk(wm.Fm(om.naive_bwt(om.rows_of(seqs, True))), True)[0], True)[0]
    stay = [s for i, s in enumerate(seqs) if kind[i] == dm.K]
    assert len(reads) - 20 < len(stay) <= len(seqs) - 6
    drop = _ok(_cli(["--pair", str(idx)], cmd="dedup"))
    u.write_bytes(_ok(_cli(["--pair", "-d", "-f", "-", str(idx)], cmd="remove", data=drop)))
    strs = om.rows_of(stay, True)
    S = dict(strs=strs, fm=wm.Fm(om.naive_bwt(strs)), key="pipeline")
    a = _model(S, True)
    assert not a["refused"] and 1 < a["n_unitigs"] < 10 and a["max_members"] > 50   # without the copies nothing branches: a few long unitigs
    um.brute_check(a, strs, L, True)
    assert _ok(_cli(["--pair", "--gfa", "-l", str(L), str(u)])) == um.gfa(a, a["seqs"])
    assert _ok(_cli(["--pair", "-l", str(L), str(u)])) == um.text(a, a["seqs"])
    rows = om.rows_of(seqs, True)
    assert _model(dict(strs=rows, fm=wm.Fm(om.naive_bwt(rows)), key="pipeline_full"), True)["refused"]
    r = _cli(["--pair", "-l", str(L), str(idx)])                                 # the copies and the contained reads are still there
    assert r.returncode == 1 and r.stdout == b"" and b"dedup --pair" in r.stderr
