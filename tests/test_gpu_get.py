"""get on the GPU: the CLI against the reference's recorded answers (tests/golden/GET_MANIFEST.json) and, on the large calls, the live reference
binary byte for byte; the Python API against the indexed records, both strands, on an index from a plain BWT, one merged from two batches and one
loaded from an FMR file -- whole and with an emit budget shorter than one string; rows out of order, twice, and outside the index."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, get_lines
from tests import util
from tests import walk_model as wm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "GET_MANIFEST.json")))
EXTRA = sorted(k for k, e in MANIFEST.items() if len(e["rows"]) > 8 or e["index"] == "longruns.fmd")


def _cli(args, timeout=300, env=None):
    return subprocess.run([CLI, "get"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)


def _args(e):
    return [os.path.join(GOLDEN, a) if a == e["index"] else a for a in e["args"]]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_matches_recorded(key):
    e = MANIFEST[key]
    r = _cli(_args(e))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.count(b"\n") == e["lines"]
    assert hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", EXTRA)
def test_cli_matches_live_reference(key):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    e = MANIFEST[key]
    ref = subprocess.run([util.REF_BIN, "get"] + _args(e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = _cli(_args(e))
    assert r.stdout == ref.stdout and r.returncode == 0


@pytest.mark.gpu
def test_cli_slices_and_missing_index(tmp_path):
    e = [x for x in MANIFEST.values() if x["index"] == "genomes12.fmd" and len(x["rows"]) == 24][0]
    r = _cli(_args(e), env=dict(os.environ, RB3GPU_GET_SLICE="50000"))      # 24 strings of 20 kbp, two or three per emit slice
    assert r.returncode == 0 and r.stdout.count(b"\n") == e["lines"] and hashlib.md5(r.stdout).hexdigest() == e["md5"]
    r = _cli([str(tmp_path / "missing.fmd"), "0"])
    assert r.returncode == 1 and r.stdout == b"" and b"failed to load index" in r.stderr


def _random_records(seed, n_genomes=4, length=2500):
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, length)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(n_genomes - 1)]
    recs.append(np.concatenate([g0[100:400], np.full(3, 5, dtype=np.uint8), g0[:200]]))   # N inside, a repeat
    recs.append(g0[:1].copy())                                                            # one symbol, and two (the host sorter takes no empty record)
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
    elif kind == "merged":            # the strings of the second batch rank behind those of the first: the rows stay in record order
        h.from_plain(host.build_bwt(util.make_text(recs[:3])))
        h.merge_plain(host.build_bwt(util.make_text(recs[3:])))
    else:                             # an FMR file written by the command's host-only `recode -b`, read back through the host library
        fmd, fmr = tmp_path / "x.fmd", tmp_path / "x.fmr"
        fmd.write_bytes(host.fmd_bytes_from_plain(host.build_bwt(util.make_text(recs)).tobytes()))
        r = subprocess.run([CLI, "recode", "-b", str(fmd)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, check=True)
        fmr.write_bytes(r.stdout)
        assert r.stdout[:3] != b"RLD"
        h.from_runs(_index_runs(fmr))
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "merged", "fmr"])
def test_api_spells_the_records(kind, tmp_path):
    rng, recs = _random_records(4)
    want = _strands(recs)
    fm = wm.Fm(host.build_bwt(util.make_text(recs)))
    h = _load(kind, recs, tmp_path)
    try:
        m = len(want)
        assert h.get_acc()[1] == m
        for budget in (None, 64):     # 64: shorter than a string, so every row is a slice of its own and the long rows exceed the budget
            if budget is not None:
                h.tune("get_slice", budget)
            st = {}
            end, seqs = h.retrieve(range(m), stats=st)
            assert len(seqs) == m and all(np.array_equal(a, b) for a, b in zip(seqs, want))
            assert len(set(end.tolist())) == m and (end >= 0).all()
            assert st["n_rows"] == m and st["n_symbols"] == sum(s.size for s in want) and st["n_steps"] == 2 * st["n_symbols"] + m + sum(1 for s in want if s.size)
            if budget is None:
                assert st["n_slices"] == 1
                if kind != "merged":  # (the same BWT: the same rows)
                    assert np.array_equal(end, fm.retrieve(np.arange(m))[0])
            else:
                assert st["n_slices"] >= m - 4    # (the rows of one and two symbols share a slice)
            # out of order, twice, a row inside a string, rows outside the index in between
            n = h.get_tot()
            rows = [5, 0, 5, -1, m + 17, 2 * m, n, 1, n - 1, 0]
            e2, s2 = h.retrieve(rows)
            for i, k in enumerate(rows):
                if 0 <= k < m:
                    assert np.array_equal(s2[i], want[k]) and e2[i] == end[k], (i, k)
                elif k < 0 or k >= n:
                    assert e2[i] == -1 and s2[i].size == 0
            if kind != "merged":
                me, ms = fm.retrieve(rows)
                assert np.array_equal(e2, me) and all(np.array_equal(a, b) for a, b in zip(s2, ms))
            assert get_lines(rows, e2, s2).count(b"\n") == 2 * sum(1 for k in rows if 0 <= k < n)
    finally:
        h.close()


@pytest.mark.gpu
def test_rows_outside_the_index_and_refusals():
    """rows outside [0, acc[6]) are answered on the host (the driver keeps them from every launch): three empty answers with end row -1"""
    rng, recs = _random_records(6, n_genomes=2, length=300)
    h, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(host.build_bwt(util.make_text(recs)))
        n = h.get_tot()
        st = {}
        end, seqs = h.retrieve([-1, n, n + 5], stats=st)
        assert end.tolist() == [-1, -1, -1] and [s.size for s in seqs] == [0, 0, 0] and st["n_steps"] == 0 and st["n_symbols"] == 0
        end, seqs = h.retrieve([])
        assert end.shape == (0,) and seqs == []
        with pytest.raises(Rb3GpuError) as e:
            empty.retrieve([0])
        assert e.value.code == -5
    finally:
        h.close()
        empty.close()


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
            end, seqs = h.retrieve(rows)
            assert all(np.array_equal(s, want[k]) for s, k in zip(seqs, rows)) and (end >= 0).all()
    finally:
        h.close()
