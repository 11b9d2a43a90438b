"""get in pieces on the GPU: `get --all` and `get --pieces` against the reference's recorded answers (tests/golden/GET_MANIFEST.json) and, on the large
calls, the live reference binary; sweeps of the splitter spacing and of the emit budget; the Python API against the indexed records, the plain path
and the model (tests/piece_model.py), its statistics included; the octet and block edges; the edge calls."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError
from tests import piece_model as pm
from tests import util
from tests import walk_model as wm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "GET_MANIFEST.json")))
EXTRA = sorted(k for k, e in MANIFEST.items() if len(e["rows"]) > 8 or e["index"] == "longruns.fmd")
ALL = [("edge_dups.fmd", 14), ("genomes12.fmd", 24), ("genomes12_first6.fmr", 12), ("longruns.fmd", 8), ("reads_fq.fmd", 6104)]


def _cli(args, timeout=300, env=None):
    return subprocess.run([CLI, "get"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)


def _args(e):
    return [os.path.join(GOLDEN, a) if a == e["index"] else a for a in e["args"]]


def _whole(idx, n):
    """the recorded call for rows 0 .. n - 1 of an index, n >= acc[1]: all of its strings (edge_dups: and two rows more)"""
    es = [e for e in MANIFEST.values() if e["index"] == idx and e["rows"] == list(range(n)) and e["acc1"] <= n]
    assert len(es) == 1 and (es[0]["acc1"] == n or "stdout" in es[0])
    return es[0]


def _same(r, e):
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.count(b"\n") == e["lines"]
    assert hashlib.md5(r.stdout).hexdigest() == e["md5"]


def _same_all(r, e):
    """`get --all` against the recorded answer for rows 0 .. : its records of the rows below acc[1], which is all of it where the call stops there"""
    if len(e["rows"]) == e["acc1"]:
        return _same(r, e)
    want = "".join(x + "\n" for x in e["stdout"].split("\n")[:2 * e["acc1"]]).encode("latin-1")
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.count(b"\n") == 2 * e["acc1"] and hashlib.md5(r.stdout).hexdigest() == hashlib.md5(want).hexdigest() and r.stdout == want


@pytest.mark.gpu
@pytest.mark.parametrize("idx,n", ALL)
def test_cli_all_matches_recorded(idx, n):
    e = _whole(idx, n)
    r = _cli(["--all", os.path.join(GOLDEN, idx)])
    _same_all(r, e)
    bre = os.path.join(GOLDEN, os.path.splitext(idx)[0] + ".bre")
    if idx in ("edge_dups.fmd", "longruns.fmd"):
        assert os.path.exists(bre)
        assert _cli(["--all", bre]).stdout == r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_pieces_matches_recorded(key):
    e = MANIFEST[key]
    _same(_cli(["--pieces"] + _args(e)), e)


@pytest.mark.gpu
@pytest.mark.parametrize("key", EXTRA)
def test_cli_pieces_matches_live_reference(key):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    e = MANIFEST[key]
    ref = subprocess.run([util.REF_BIN, "get"] + _args(e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = _cli(["--pieces"] + _args(e))
    assert r.stdout == ref.stdout and r.returncode == 0


def _sweep_cases():
    """the genomes12 call of 24 strings, the edge_dups call of 14, and every call on k2_fwd"""
    ks = [k for k, e in MANIFEST.items() if (e["index"], len(e["rows"])) in (("genomes12.fmd", 24), ("edge_dups.fmd", 14)) or e["index"] == "k2_fwd.fmd"]
    assert len(ks) >= 4
    return sorted(ks)


@pytest.mark.gpu
@pytest.mark.parametrize("var,val", [("RB3GPU_GET_PIECE", "1"), ("RB3GPU_GET_PIECE", "2"), ("RB3GPU_GET_PIECE", "3"), ("RB3GPU_GET_PIECE", "20"),
                                     ("RB3GPU_GET_SLICE", "64"), ("RB3GPU_GET_SLICE", "50000")])
def test_cli_spacing_and_slice_sweeps(var, val):
    """spacings of 2, 4 and 8 rows: pieces of a few steps; 20: row acc[1] is the only splitter that is no sentinel row; a budget of 64: every string
    a slice of its own and longer than the budget"""
    env = dict(os.environ, **{var: val})
    for key in _sweep_cases():
        e = MANIFEST[key]
        _same(_cli(["--pieces"] + _args(e), env=env), e)
        if len(e["rows"]) > 8:
            _same_all(_cli(["--all", os.path.join(GOLDEN, e["index"])], env=env), e)


@pytest.mark.gpu
def test_cli_verbose_line_names_the_pieces():
    e = _whole("edge_dups.fmd", 14)
    r = _cli(["--all", os.path.join(GOLDEN, "edge_dups.fmd")], env=dict(os.environ, RB3_VERBOSE="3", RB3GPU_GET_PIECE="2"))
    _same_all(r, e)
    line = [x for x in r.stderr.decode().splitlines() if "main_get" in x][-1]
    n_pieces = e["acc1"] + -(-(e["acc6"] - e["acc1"]) // 4)
    assert "%d pieces, the longest of " % n_pieces in line and all(w in line for w in ("pieces ", "join ", "sort ", "writing walk "))


# ---- the API (the helpers of tests/test_gpu_get.py, restated) ----

def _random_records(seed, n_genomes=4, length=2500):
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, length)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(n_genomes - 1)]
    recs.append(np.concatenate([g0[100:400], np.full(3, 5, dtype=np.uint8), g0[:200]]))   # N inside, a repeat
    recs.append(g0[:1].copy())                                                            # one symbol, and two
    recs.append(g0[7:9].copy())
    return rng, recs


def _strands(recs):
    out = []
    for s in recs:
        out += [np.asarray(s, dtype=np.uint8), util.revcomp(np.asarray(s, dtype=np.uint8))]
    return out


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


def _load(kind, recs, tmp_path):
    h = Rb3Gpu(verbose=1)
    if kind == "plain":
        h.from_plain(host.build_bwt(util.make_text(recs)))
    elif kind == "merged":
        h.from_plain(host.build_bwt(util.make_text(recs[:3])))
        h.merge_plain(host.build_bwt(util.make_text(recs[3:])))
    else:
        fmd, fmr = tmp_path / "x.fmd", tmp_path / "x.fmr"
        fmd.write_bytes(host.fmd_bytes_from_plain(host.build_bwt(util.make_text(recs)).tobytes()))
        r = subprocess.run([CLI, "recode", "-b", str(fmd)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, check=True)
        fmr.write_bytes(r.stdout)
        assert r.stdout[:3] != b"RLD"
        h.from_runs(_index_runs(fmr))
    return h


_REF = {}


def _reference():
    """the records, their strands and the model's index: computed once, shared, never changed"""
    if not _REF:
        rng, recs = _random_records(4)
        _REF.update(recs=recs, want=_strands(recs), fm=wm.Fm(host.build_bwt(util.make_text(recs))), pc={})
    return _REF


def _eq(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "merged", "fmr"])
def test_api_spells_the_records(kind, tmp_path):
    R = _reference()
    recs, want, fm = R["recs"], R["want"], R["fm"]
    h = _load(kind, recs, tmp_path)
    try:
        m, n = len(want), h.get_tot()
        assert h.get_acc()[1] == m and n == fm.n
        end0, seqs0 = h.retrieve(range(m))
        assert _eq(seqs0, want)
        for S in (1, 3, 8):
            h.tune("get_piece", S)
            if S not in R["pc"]:
                R["pc"][S] = pm.Pieces(fm, S)
            pc = R["pc"][S]
            st, sa = {}, {}
            end, seqs = h.retrieve(range(m), stats=st, pieces=True)
            enda, seqsa = h.retrieve_all(stats=sa)
            assert _eq(seqs, want) and _eq(seqsa, want) and np.array_equal(end, end0) and np.array_equal(enda, end0)
            # rows out of order, twice, inside a string, outside the index; splitter rows asked for themselves; a row that reads the sentinel before any splitter
            cand = np.arange(m, n, dtype=np.int64)
            cand = cand[~pc.is_split(cand)]
            nxt, _, steps = pc._walk(cand, False)
            short = cand[nxt < 0][np.argsort(-steps[nxt < 0], kind="stable")]
            inner = short[:2].tolist() + short[-1:].tolist()     # the longest such walks and one that reads the sentinel at once
            assert len(inner) == 3 and steps[nxt < 0].min() == 1 and (S == 1 or steps[nxt < 0].max() > 2)
            for rows in ([5, 0, 5, -1, m + 17, 2 * m, n, 1, n - 1, 0], [m, m + (1 << S), 3, m + 1, m, m + (2 << S)] + inner):
                s2 = {}
                e1, q1 = h.retrieve(rows)
                e2, q2 = h.retrieve(rows, stats=s2, pieces=True)
                assert np.array_equal(e1, e2) and _eq(q1, q2), (S, rows)
                if kind != "merged":          # (the same BWT: the same rows, pieces and steps)
                    me, mq, ms = pc.retrieve(rows)
                    assert np.array_equal(e2, me) and _eq(q2, mq)
                    assert {k: s2[k] for k in ms} == ms, (S, rows)
            assert st["n_pieces"] == sa["n_pieces"] == m + -(-(n - m) // (1 << S))
            assert st["n_symbols"] == sa["n_symbols"] == sum(s.size for s in want) and st["n_rows"] == sa["n_rows"] == m
            if kind != "merged":
                ms = pc.retrieve(range(m))[2]
                assert {k: st[k] for k in ms} == ms and {k: sa[k] for k in ms} == ms
        h.tune("get_piece", 3)
        h.tune("get_slice", 64)               # shorter than a string: every long row a slice of its own
        st = {}
        end, seqs = h.retrieve_all(stats=st)
        assert _eq(seqs, want) and np.array_equal(end, end0) and st["n_slices"] >= m - 4
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 300])
def test_octets_of_a_wave_and_of_a_block(n):
    """9 rows: one octet more than a wave holds; 300: more than the 32 octets of a block.  150 reads of lengths from 1 to 120, both strands"""
    rng = np.random.default_rng(8)
    g0 = util.random_genome(rng, 3000)
    reads = [g0[s:s + 1 + (i * 7) % 120].copy() for i, s in enumerate(rng.integers(0, 2800, size=150))]
    want = _strands(reads)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(util.make_text(reads)))
        rows = rng.permutation(300)[:n]
        for budget in (0, 500):
            h.tune("get_slice", budget)
            end, seqs = h.retrieve(rows, pieces=True)
            assert all(np.array_equal(s, want[k]) for s, k in zip(seqs, rows)) and (end >= 0).all()
            if n == 300:
                assert _eq(h.retrieve_all()[1], want)
    finally:
        h.close()


@pytest.mark.gpu
def test_edge_calls():
    rng, recs = _random_records(6, n_genomes=2, length=300)
    h, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(host.build_bwt(util.make_text(recs)))
        n = h.get_tot()
        st = {}
        end, seqs = h.retrieve([-1, n, n + 5], stats=st, pieces=True)
        assert end.tolist() == [-1, -1, -1] and [s.size for s in seqs] == [0, 0, 0] and st["n_symbols"] == 0 and st["n_steps"] == 0 and st["n_rows"] == 3
        end, seqs = h.retrieve([], pieces=True)
        assert end.shape == (0,) and seqs == []
        for call in (lambda: empty.retrieve([0], pieces=True), empty.retrieve_all):
            with pytest.raises(Rb3GpuError) as e:
                call()
            assert e.value.code == -5
    finally:
        h.close()
        empty.close()
