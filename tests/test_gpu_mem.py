"""mem on the GPU: the CLI against the reference's recorded answers (tests/golden/MEM_MANIFEST.json) and, outside the regular matrix, the
live reference binary byte for byte; its refusals; the Python API against the string model (tests/mem_model.py); chunk independence --
the same records whatever the walkers' chunk -- on the mutated 20 kbp queries and on one mutated 600 kbp query against an index built
through the merge path; a call cut into output slices."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, mem_lines
from tests import util
from tests import kount_model as km
from tests import mem_model as mm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MEM_MANIFEST.json")))
EXTRA = sorted(k for k, e in MANIFEST.items() if not e["matrix"])
WHOLE = 2 ** 31 - 1   # a chunk no query exceeds: one walker per query


def _cli(args, timeout=300):
    return subprocess.run([CLI, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


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
    ref = subprocess.run([util.REF_BIN, "mem"] + _args(e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = _cli(_args(e))
    assert r.stdout == ref.stdout
    assert r.returncode == (1 if "refused" in e else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["7", "100", "1m"])
def test_cli_chunk_option_changes_nothing(chunk):
    e = MANIFEST["-l19 -c2 genomes12.fmd mem_mutated.fa.gz"]
    r = _cli(["--chunk", chunk] + _args(e))
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
def test_cli_refusals(tmp_path):
    idx, q = os.path.join(GOLDEN, "genomes12.fmd"), os.path.join(GOLDEN, "mem_iupac.fa")
    for bad in (["-p", "5"], ["--old-mem"], ["-l0"], ["-c0"], ["-d"], ["-N", "5"]):
        r = _cli(bad + [idx, q])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1, bad
    r = _cli([str(tmp_path / "missing.fmd"), q])
    assert r.returncode == 1 and r.stdout == b"" and b"failed to load index" in r.stderr
    r = _cli([idx, q, str(tmp_path / "missing.fa")])   # (the queries before the missing file are answered)
    assert r.returncode == 1 and b"failed to load the sequence file" in r.stderr and r.stdout.count(b"\n") == MANIFEST["-l19 -c1 genomes12.fmd mem_iupac.fa"]["lines"]


def _random_index(seed, n_genomes=4, length=2500):
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, length)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(n_genomes - 1)]
    recs.append(np.concatenate([g0[100:400], np.full(3, 5, dtype=np.uint8), g0[:200]]))   # N inside, a repeat
    return rng, g0, recs


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_api_matches_model(seed):
    rng, g0, recs = _random_index(seed)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(util.make_text(recs)))
        text = mm.Text(mm.both_strands(recs))
        queries = [util.mutate(rng, g0, 0.03), util.revcomp(util.mutate(rng, g0[500:1500], 0.01)), np.full(30, 5, dtype=np.uint8), g0[:10], np.zeros(0, dtype=np.uint8),
                   util.random_genome(rng, 300), np.concatenate([g0[:50], np.full(1, 5, dtype=np.uint8), g0[50:120]])]
        for l, c in [(19, 1), (1, 1), (1, 3), (5, 2), (12, 5), (31, 2), (2000, 1)]:
            want = mm.mem(text, queries, l, c)
            for chunk in (None, 16, WHOLE):
                st = {}
                got = h.mem(queries, l, c, chunk=chunk, stats=st)
                assert got.shape == want.shape, (l, c, chunk)
                for f in ("query", "st", "en", "size"):
                    assert np.array_equal(got[f], want[f]), (l, c, chunk, f)
                assert st["n_records"] == want.shape[0] and st["n_slices"] >= 1
            assert mem_lines(got, names=["a", None, "c", None, None, "f", "g"], first_id=10) == mm.lines(want, ["a", None, "c", None, None, "f", "g"], 10)
        assert np.array_equal(h.mem(["ACGTNacgtn", b"RYKM"], 1, 1)["st"], h.mem([np.array([1, 2, 3, 4, 5, 1, 2, 3, 4, 5]), np.array([5, 5, 5, 5])], 1, 1)["st"])
    finally:
        h.close()


@pytest.mark.gpu
def test_api_refusals():
    h = Rb3Gpu(verbose=0)
    fwd = Rb3Gpu(verbose=0)
    empty = Rb3Gpu(verbose=0)
    try:
        h.from_plain(km.golden_plain(GOLDEN, "k4_readme.fmd", CLI))
        fwd.from_plain(km.golden_plain(GOLDEN, "k2_fwd.fmd", CLI))
        for l, c in ((0, 1), (-1, 1), (19, 0)):
            with pytest.raises(Rb3GpuError) as e:
                h.mem(["ACGT"], l, c)
            assert e.value.code == -3
        for x in (fwd, empty):
            with pytest.raises(Rb3GpuError) as e:
                x.mem(["ACGT"], 19, 1)
            assert e.value.code == -5
        assert h.mem([], 19, 1).shape == (0,) and h.mem(["", ""], 19, 1).shape == (0,) and h.mem(["ACGT"], 19, 1).shape == (0,)
    finally:
        for x in (h, fwd, empty):
            x.close()


def _same(a, b):
    return a.shape == b.shape and all(np.array_equal(a[f], b[f]) for f in ("query", "x0", "size", "st", "en"))


@pytest.mark.gpu
@pytest.mark.parametrize("l,c", [(19, 1), (19, 2), (5, 3), (31, 9), (1, 1)])
def test_chunk_independence_mutated_queries(l, c):
    """the mutated 20 kbp queries on genomes12: the same records for walkers of 8, 64 and 1000 symbols and one walker per query, more than one
    walker per query in the chunked runs, and the text equals the recorded reference output where the manifest has the case"""
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(km.golden_plain(GOLDEN, "genomes12.fmd", CLI))
        qs = mm.read_queries(os.path.join(GOLDEN, "mem_mutated.fa.gz"))
        st = {}
        whole = h.mem([s for _, s in qs], l, c, chunk=WHOLE, stats=st)
        assert st["n_walkers"] == len(qs) and whole.shape[0] > 0
        for chunk in (8, 64, 1000, None):
            st = {}
            got = h.mem([s for _, s in qs], l, c, chunk=chunk, stats=st)
            assert _same(got, whole), chunk
            assert st["n_walkers"] > len(qs) * 2
        key = "-l%d -c%d genomes12.fmd mem_mutated.fa.gz" % (l, c)
        if key in MANIFEST:
            assert hashlib.md5(mem_lines(whole, [n for n, _ in qs])).hexdigest() == MANIFEST[key]["md5"]
        h.tune("mem_slice", 3000)   # the same call in output slices of 3000 query symbols
        st = {}
        got = h.mem([s for _, s in qs], l, c, chunk=64, stats=st)
        assert _same(got, whole) and st["n_slices"] > 10
    finally:
        h.close()


@pytest.mark.gpu
def test_cli_sliced_output_same_bytes():
    e = MANIFEST["-l5 -c2 genomes12.fmd mem_mutated.fa.gz"]
    env = dict(os.environ, RB3GPU_MEM_SLICE="1000")
    r = subprocess.run([CLI, "mem"] + _args(e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.count(b"\n") == e["lines"] and hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
def test_scale_merged_index_long_query():
    """an index of ~4.8 M symbols built in four batches through the merge path; one mutated 600 kbp query: the same records for walkers of 8,
    64 and 1000 symbols, the default and ONE walker for the whole query, and in output slices; a sample of the matches checked on the strings"""
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
        q = util.mutate(rng, g0, 0.01)
        q[300000:300040] = 5
        st = {}
        whole = h.mem([q], 19, 1, chunk=WHOLE, stats=st)
        assert st["n_walkers"] == 1 and whole.shape[0] > 3000
        for chunk in (8, 64, 1000, None):
            st = {}
            got = h.mem([q], 19, 1, chunk=chunk, stats=st)
            assert _same(got, whole), chunk
            assert st["n_walkers"] > 100 and st["n_steps"] > q.size
        h.tune("mem_slice", 50000)
        st = {}
        got = h.mem([q, q[:1000], q], 19, 1, stats=st)
        assert st["n_slices"] > 20
        assert _same(got[got["query"] == 0], whole) and np.array_equal(got[got["query"] == 2]["st"], whole["st"])
        # a sample of the matches against the strings: it occurs `size` times, and neither extension by one symbol occurs at all
        hay = b"".join(bytes(bytearray(t.tolist())) for t in texts)
        for r in whole[rng.choice(whole.shape[0], size=40, replace=False)]:
            s, e = int(r["st"]), int(r["en"])
            assert e - s >= 19 and _count(hay, bytes(bytearray(q[s:e].tolist()))) == r["size"]
            assert s == 0 or _count(hay, bytes(bytearray(q[s - 1:e].tolist()))) == 0
            assert e == q.size or _count(hay, bytes(bytearray(q[s:e + 1].tolist()))) == 0
    finally:
        h.close()


def _count(hay, p):
    n, i = 0, hay.find(p)
    while i >= 0:
        n, i = n + 1, hay.find(p, i + 1)
    return n
