"""kount on the GPU: the CLI against the reference's recorded answers (tests/golden/KOUNT_MANIFEST.json) and the live reference binary
byte for byte, its refusals, the Python API against the model (tests/kount_model.py), a walk cut into slices, and an index built
through the merge path whose frontier holds more than a million nodes."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, kount_lines
from tests import util
from tests import kount_model as km

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "KOUNT_MANIFEST.json")))
# the cases beyond the matrix of every index at k in {1, 3, 31, 51, 80} and m in {1, 2, 100}: also run against the live reference
EXTRA = sorted(key for key, e in MANIFEST.items() if not (len(e["args"]) == 3 and e["args"][0] in ("-k1", "-k3", "-k31", "-k51", "-k80")
                                                        and e["args"][1] in ("-m1", "-m2", "-m100")))


def _cli(args, timeout=120):
    return subprocess.run([CLI, "kount"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def _paths(args):
    return args[:2] + [os.path.join(GOLDEN, f) for f in args[2:]]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_matches_recorded(key):
    e = MANIFEST[key]
    r = _cli(_paths(e["args"]))
    assert r.returncode == e["exit"] == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.count(b"\n") == e["lines"]
    assert hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", EXTRA)
def test_cli_matches_live_reference(key):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    args = _paths(MANIFEST[key]["args"])
    ref = subprocess.run([util.REF_BIN, "kount"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = _cli(args)
    assert r.returncode == ref.returncode == 0
    assert r.stdout == ref.stdout


@pytest.mark.gpu
def test_cli_edge_cases(tmp_path):
    r = _cli(_paths(["-k12", "-m1000000000", "genomes12.fmd"]))
    assert r.returncode == 0 and r.stdout == b""
    r = _cli(_paths(["-k0", "-m1", "k4_readme.fmd"]))
    assert r.returncode == 1 and r.stdout == b""
    r = _cli(["-k3", str(tmp_path / "missing.fmd")])
    assert r.returncode == 1 and r.stdout == b"" and b"failed to load index" in r.stderr
    r = _cli(_paths(["-k3", "-m1", "k4_readme.fmd"]) + [str(tmp_path / "missing.fmd")])
    assert r.returncode == 1 and r.stdout == b""
    r = _cli(_paths(["-k6", "-m0", "k2_fwd.fmd"]))
    assert r.returncode == 0 and r.stdout.count(b"\n") == 4096


def _load(name):
    h = Rb3Gpu(verbose=1)
    plain = km.golden_plain(GOLDEN, name, CLI)
    h.from_plain(plain)
    return h, plain


@pytest.mark.gpu
@pytest.mark.parametrize("names,k,m", [(["reads_fq.fmd"], 51, 2), (["genomes12.fmd"], 80, 1), (["k4_readme.fmd"], 7, 0),
                                       (["reads_fwd.fmd", "reads_rev.fmd"], 17, 3), (["genomes12_first6.fmr", "reads_fq.fmd", "edge_chars.fmd"], 25, 2)])
def test_api_matches_model(names, k, m):
    hs = [_load(f) for f in names]
    try:
        st = {}
        kmers, counts = hs[0][0].kount(k, m, others=[h for h, _ in hs[1:]], stats=st)
        wk, wc = km.kount([p for _, p in hs], k, m)
        assert kmers.shape == wk.shape and counts.shape == wc.shape
        assert np.array_equal(kmers, wk) and np.array_equal(counts, wc)
        assert st["n_out"] == wk.shape[0] and st["n_slices"] == 1 and st["n_nodes"] > 0
        if wk.shape[0] < 5000:
            assert kount_lines(kmers, counts) == km.lines(wk, wc)
    finally:
        for h, _ in hs:
            h.close()


@pytest.mark.gpu
def test_api_refusals():
    h, _ = _load("k4_readme.fmd")
    empty = Rb3Gpu(verbose=0)
    try:
        for k in (0, -1):
            with pytest.raises(Rb3GpuError) as e:
                h.kount(k, 1)
            assert e.value.code == -3
        with pytest.raises(Rb3GpuError) as e:
            h.kount(3, 1, others=[empty])
        assert e.value.code == -5
        k, c = h.kount(3, 10 ** 9)
        assert k.shape == (0, 3) and c.shape == (0, 1)
    finally:
        empty.close()
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 7, 1000])
@pytest.mark.parametrize("names,k,m", [(["genomes12.fmd"], 31, 2), (["reads_fwd.fmd", "edge_chars.fmd"], 12, 1)])
def test_sliced_walk_same_output(cap, names, k, m):
    hs = [_load(f) for f in names]
    try:
        others = [h for h, _ in hs[1:]]
        want = hs[0][0].kount(k, m, others=others)
        st = {}
        got = hs[0][0].kount(k, m, others=others, max_level_nodes=cap, stats=st)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert st["n_slices"] > 1
    finally:
        for h, _ in hs:
            h.close()


@pytest.mark.gpu
def test_scale_merged_index_million_node_level():
    """an index of ~4.8 M symbols built in four batches through the merge path; at k = 24, m = 1 the deepest frontiers hold millions of
    nodes (nearly every 24-mer of a random genome is unique); the result equals the model, whole and in slices"""
    rng = np.random.default_rng(11)
    g0 = util.random_genome(rng, 600000)
    h = Rb3Gpu(verbose=1)
    try:
        batches = [[g0], [util.mutate(rng, g0, 0.01)], util.reads_from(rng, g0, 4000, 150, err=0.01), [util.mutate(rng, g0, 0.003)]]
        texts = [util.make_text(b) for b in batches]
        h.from_plain(host.build_bwt(texts[0].copy()))
        for t in texts[1:]:
            h.merge_plain(host.build_bwt(t.copy()))
        assert h.get_tot() > 4_000_000
        st = {}
        kmers, counts = h.kount(24, 1, stats=st)
        wk, wc = km.kount_strings([[s for t in texts for s in km.strings_of_text(t)]], 24, 1)  # (the strings the index was built from)
        assert np.array_equal(kmers, wk) and np.array_equal(counts, wc)
        assert wk.shape[0] > 1_000_000 and st["n_out"] == wk.shape[0]
        st2 = {}
        k2, c2 = h.kount(24, 2, max_level_nodes=300000, stats=st2)
        w2 = (wk[wc[:, 0] >= 2], wc[wc[:, 0] >= 2])
        assert st2["n_slices"] > 1
        assert np.array_equal(k2, w2[0]) and np.array_equal(c2, w2[1])
    finally:
        h.close()
