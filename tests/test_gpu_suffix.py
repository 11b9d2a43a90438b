"""suffix on the GPU: the CLI against the reference's recorded answers (tests/golden/SUFFIX_MANIFEST.json) and, outside the regular matrix, the live
reference binary byte for byte; the Python API against the walk restated in tests/walk_model.py on a random index, whole and in slices of three
queries; one octet more than a wave holds, and more queries than a block has octets."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, suffix_lines
from tests import util
from tests import walk_model as wm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "SUFFIX_MANIFEST.json")))
EXTRA = sorted(k for k, e in MANIFEST.items() if not e["matrix"])


def _cli(args, timeout=300, env=None):
    return subprocess.run([CLI, "suffix"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)


def _args(e):
    return e["opts"] + [os.path.join(GOLDEN, f) for f in e["files"]]


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
    ref = subprocess.run([util.REF_BIN, "suffix"] + _args(e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = _cli(_args(e))
    assert r.stdout == ref.stdout and r.returncode == 0


@pytest.mark.gpu
def test_cli_slices_and_missing_files(tmp_path):
    e = MANIFEST["reads_fq.fmd reads_fq.fa.gz"]
    r = _cli(_args(e), env=dict(os.environ, RB3GPU_SUFFIX_SLICE="100"))     # 3052 queries, 100 per launch
    assert r.returncode == 0 and r.stdout.count(b"\n") == e["lines"] and hashlib.md5(r.stdout).hexdigest() == e["md5"]
    idx, q = os.path.join(GOLDEN, "genomes12.fmd"), os.path.join(GOLDEN, "mem_iupac.fa")
    r = _cli([str(tmp_path / "missing.fmd"), q])
    assert r.returncode == 1 and r.stdout == b"" and b"failed to load index" in r.stderr
    r = _cli([idx, q, str(tmp_path / "missing.fa"), q])   # (the queries before the missing file are answered, those behind it are not)
    assert r.returncode == 1 and b"failed to load the sequence file" in r.stderr and r.stdout.decode() == MANIFEST["genomes12.fmd mem_iupac.fa"]["stdout"]


def _random_index(seed, n_genomes=4, length=2500):
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, length)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(n_genomes - 1)]
    recs.append(np.concatenate([g0[100:400], np.full(3, 5, dtype=np.uint8), g0[:200]]))   # N inside, a repeat
    return rng, g0, recs


def _same(got, want):
    start, length, size = want
    return (np.array_equal(got["query"], np.arange(len(start))) and np.array_equal(got["start"], start) and np.array_equal(got["length"], length)
            and np.array_equal(got["size"], size))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_api_matches_model(seed):
    rng, g0, recs = _random_index(seed)
    bwt = host.build_bwt(util.make_text(recs))
    fm = wm.Fm(bwt)
    queries = [util.mutate(rng, g0, 0.03), util.revcomp(util.mutate(rng, g0[500:1500], 0.01)), np.full(30, 5, dtype=np.uint8), g0[:10], g0[7:8], np.zeros(0, dtype=np.uint8),
               util.random_genome(rng, 300), recs[2].copy()]
    want = fm.suffix(queries)
    assert want[0][7] == 0 and want[2][7] >= 1 and (want[0][2], want[2][2]) == (27, 2) and 0 < want[0][0] < 2500   # the copy whole, NNN of the Ns (both strands), the mutated genome in part
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(bwt)
        st = {}
        whole = h.suffix(queries, stats=st)
        assert _same(whole, want)
        assert st["n_queries"] == len(queries) and st["n_slices"] == 1 and st["n_symbols"] == sum(q.size for q in queries)
        assert st["n_steps"] == int(np.sum(np.minimum(want[1] - want[0] + 1, want[1])))          # one step per symbol taken and one for the symbol that failed
        h.tune("suffix_slice", 3)
        st = {}
        got = h.suffix(queries, stats=st)
        assert _same(got, want) and st["n_slices"] == 3
        names = ["a", None, "c", None, None, "f", "g", None]
        assert suffix_lines(got, names, first_id=10) == b"".join(b"%s\t%d\t%d\t%d\n" % (n.encode() if n else b"seq%d" % (11 + i), want[0][i], want[1][i], want[2][i])
                                                               for i, n in enumerate(names))
        a = h.suffix(["ACGTNacgtn", b"RYKM", ""])
        b = h.suffix([np.array([1, 2, 3, 4, 5, 1, 2, 3, 4, 5]), np.array([5, 5, 5, 5]), np.zeros(0, dtype=np.uint8)])
        assert all(np.array_equal(a[f], b[f]) for f in ("start", "length", "size"))
        assert h.suffix([]).shape == (0,) and h.suffix(["", ""])["size"].tolist() == [0, 0]
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 300])
def test_octets_of_a_wave_and_of_a_block(n):
    """9 queries: one octet more than a wave holds; 300: more than the 32 octets of a block (one block of them would take queries from the counter
    ten times over).  Reads of every length from 0 to 120, half of them with an error"""
    rng, g0, recs = _random_index(3)
    bwt = host.build_bwt(util.make_text(recs))
    queries = []
    for i in range(n):
        s = int(rng.integers(0, 2300))
        q = g0[s:s + (i * 7) % 121].copy()
        if i & 1 and q.size:
            q[int(rng.integers(0, q.size))] = 5
        queries.append(q)
    want = wm.Fm(bwt).suffix(queries)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(bwt)
        assert _same(h.suffix(queries), want)
        h.tune("suffix_slice", 7)
        assert _same(h.suffix(queries), want)
    finally:
        h.close()


@pytest.mark.gpu
def test_forward_only_index_and_refusals():
    """an index of one strand serves (mem refuses it); a handle without an index does not"""
    rng = np.random.default_rng(5)
    recs = [util.random_genome(rng, 400) for _ in range(3)]
    bwt = host.build_bwt(util.make_text(recs, rev=False))
    queries = [recs[1][100:300], util.revcomp(recs[1][100:300]), recs[2]]
    want = wm.Fm(bwt).suffix(queries)
    h, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(bwt)
        assert _same(h.suffix(queries), want) and want[0][0] == 0 and want[0][1] > 100
        with pytest.raises(Rb3GpuError) as e:
            empty.suffix(["ACGT"])
        assert e.value.code == -5
    finally:
        h.close()
        empty.close()
