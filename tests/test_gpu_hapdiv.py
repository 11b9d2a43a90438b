"""hapdiv on the GPU: the CLI against the reference's recorded answers (tests/golden/HAPDIV_MANIFEST.json) and, outside the regular
matrix, the live reference binary byte for byte; the Python API against the model of the dynamic program (tests/sw_model.py) on random
indexes; the same bytes in many slices, with every table in global memory, and on an index built through the merge path; the refusals."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, hapdiv_lines
from tests import util
from tests import kount_model as km
from tests import mem_model as mm
from tests import sw_model as sw

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "HAPDIV_MANIFEST.json")))
EXTRA = sorted(k for k, e in MANIFEST.items() if not e["matrix"])
DEFAULT = "genomes12.fmd mem_mutated.fa.gz"


def _cli(args, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI, "hapdiv"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=e)


def _args(e):
    return e["opts"] + [os.path.join(GOLDEN, f) for f in e["files"]]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_matches_recorded(key):
    e = MANIFEST[key]
    r = _cli(_args(e))
    if "refused" in e:   # forward-only index: the reference's message, nothing on stdout (and exit 1 here)
        assert r.returncode == 1 and r.stdout == b"" and e["refused"].encode() in r.stderr
        return
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.count(b"\n") == e["lines"]
    assert hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", EXTRA)
def test_cli_matches_live_reference(key):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    e = MANIFEST[key]
    ref = subprocess.run([util.REF_BIN, "hapdiv"] + _args(e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = _cli(_args(e))
    assert r.stdout == ref.stdout
    assert r.returncode == (1 if "refused" in e else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("key", [DEFAULT, "-a51 -w10 -N5 " + DEFAULT, "-N200 " + DEFAULT, "-a31 -w7 reads_fq.fmd reads_fq.fa.gz"])
def test_cli_slices_and_global_tables_change_nothing(key):
    e = MANIFEST[key]
    for env in ({"RB3GPU_HAPDIV_SLICE": "37"}, {"RB3GPU_HAPDIV_TABLE": "1"}, {"RB3GPU_HAPDIV_TABLE": "128", "RB3GPU_HAPDIV_SLICE": "500"}):
        r = _cli(_args(e), env)
        assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == e["md5"], env


@pytest.mark.gpu
def test_cli_refusals(tmp_path):
    idx, q = os.path.join(GOLDEN, "genomes12.fmd"), os.path.join(GOLDEN, "mem_iupac.fa")
    for bad in (["-a0"], ["-w0"], ["-N0"], ["-a", "-3"], ["-p", "5"], ["-d"], ["-g", "10"], ["--gap=20"], ["--cov"], ["--old-mem"], ["--all-e2e"]):
        r = _cli(bad + [idx, q])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1, bad
    r = _cli([str(tmp_path / "missing.fmd"), q])
    assert r.returncode == 1 and r.stdout == b"" and b"failed to load index" in r.stderr
    r = _cli(["-e", "-k", "5", "-b", "-u", "-j", "30", "-l", "40", "--seq", "-t", "3", "-C", "1k", idx, q])   # accepted and ignored
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == MANIFEST["genomes12.fmd mem_iupac.fa"]["md5"]
    u = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"hapdiv" in u.stdout + u.stderr


def _random_index(seed, n_genomes=4, length=2500):
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, length)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(n_genomes - 1)]
    recs.append(np.concatenate([g0[100:400], np.full(3, 5, dtype=np.uint8), g0[:200]]))   # N inside, a repeat
    return rng, g0, recs


def _model_recs(ix, queries, k, w, opt):
    wins = sw.hapdiv(ix, queries, k, w, opt)
    return np.array([x[2] for x in wins], dtype=np.int32).reshape(-1, 9), np.array([x[:2] for x in wins], dtype=np.int64).reshape(-1, 2), wins


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_api_matches_model(seed):
    rng, g0, recs = _random_index(seed)
    h = Rb3Gpu(verbose=1)
    try:
        bwt = host.build_bwt(util.make_text(recs))
        h.from_plain(bwt)
        ix = sw.BwtIndex(h.export_plain())
        queries = [util.mutate(rng, g0[:700], 0.03), util.revcomp(util.mutate(rng, g0[500:1100], 0.02)), np.full(60, 5, dtype=np.uint8), g0[:10], np.zeros(0, dtype=np.uint8),
                   util.random_genome(rng, 120), np.concatenate([g0[:50], np.full(1, 5, dtype=np.uint8), g0[50:120]])]
        names = ["a", None, "c", None, None, "f", "g"]
        for n_best in (1, 4, 25):
            for k, w, extra in ((41, 17, {}), (25, 25, {"min_sc": 10, "e2e_drop": 3}), (33, 40, {"match": 2, "mis": 4, "gap_open": 4, "gap_ext": 1})):
                opt = dict(extra, n_best=n_best)
                want, where, wins = _model_recs(ix, queries, k, w, opt)
                st = {}
                got, gw = h.hapdiv(queries, k, w, stats=st, **opt)
                assert np.array_equal(gw, where) and np.array_equal(got, want), (n_best, k, w)
                assert st["n_windows"] == want.shape[0] and st["n_ext"] > 0 and st["n_slices"] == 1
                assert hapdiv_lines(got, gw, k, names, first_id=10) == sw.merge_lines(wins, k, names, 10)
        assert want[:, 0].max() > 0
        h.tune("hapdiv_slice", 5)          # many slices; every table in global memory
        h.tune("hapdiv_table", 1)
        st = {}
        again, _ = h.hapdiv(queries, k, w, stats=st, **opt)
        assert np.array_equal(again, want) and st["n_slices"] > 5 and st["n_tier2"] == st["n_windows"]
    finally:
        h.close()


@pytest.mark.gpu
def test_merged_index_gives_the_same_bytes():
    """the index of the twelve genomes built in two batches through the merge path answers as the one loaded from the file"""
    e = MANIFEST["-a51 -w10 -N5 " + DEFAULT]
    qs = mm.read_queries(os.path.join(GOLDEN, "mem_mutated.fa.gz"))
    a = km.golden_plain(GOLDEN, "genomes12_first6.fmd", CLI)
    h, other = Rb3Gpu(verbose=1), Rb3Gpu(verbose=1)
    try:
        recs = [s for s in km.strings_of(a)]
        half = len(recs) // 2
        h.from_plain(host.build_bwt(_text(recs[:half])))
        h.merge_plain(host.build_bwt(_text(recs[half:])))
        other.from_plain(a)
        for n_best in (5, 25):
            x, wx = h.hapdiv([s for _, s in qs], 51, 10, n_best=n_best)
            y, wy = other.hapdiv([s for _, s in qs], 51, 10, n_best=n_best)
            assert np.array_equal(x, y) and np.array_equal(wx, wy) and x[:, 0].max() > 0
        whole = Rb3Gpu(verbose=1)
        try:
            whole.from_plain(km.golden_plain(GOLDEN, "genomes12.fmd", CLI))
            z, wz = whole.hapdiv([s for _, s in qs], 51, 10, n_best=5)
            assert hashlib.md5(hapdiv_lines(z, wz, 51, [n for n, _ in qs])).hexdigest() == e["md5"]
        finally:
            whole.close()
    finally:
        h.close()
        other.close()


def _text(strings):
    """the strings as they are (both strands are among them already), each ended by a sentinel"""
    parts = []
    for s in strings:
        parts += [np.asarray(s, dtype=np.uint8), np.zeros(1, dtype=np.uint8)]
    return np.concatenate(parts)


@pytest.mark.gpu
def test_api_refusals():
    h, fwd, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(km.golden_plain(GOLDEN, "k4_readme.fmd", CLI))
        fwd.from_plain(km.golden_plain(GOLDEN, "k2_fwd.fmd", CLI))
        with pytest.raises(Rb3GpuError) as e:
            h.hapdiv(["ACGTACGT"], 4, 1, n_best=0)
        assert e.value.code == -3
        with pytest.raises(ValueError):
            h.hapdiv(["ACGTACGT"], 0, 1)
        for x in (fwd, empty):
            with pytest.raises(Rb3GpuError) as e:
                x.hapdiv(["ACGTACGT"], 4, 1)
            assert e.value.code == -5
        got, where = h.hapdiv(["ACG", "", "ACGTA"], 4, 1, min_sc=1)
        assert got.shape == (2, 9) and where.tolist() == [[2, 0], [2, 1]]
        assert h.hapdiv([], 4, 1)[0].shape == (0, 9)
    finally:
        for x in (h, fwd, empty):
            x.close()
