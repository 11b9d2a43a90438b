"""sw --local on the GPU: the CLI against the reference's recorded answers (tests/golden/SWLOCAL_MANIFEST.json: the reference's options, with
`--local` in front) and, outside the regular matrix, the live reference binary byte for byte; the Python API against the model
(tests/swlocal_model.py) on a small random index at the query lengths and -N where the kernel takes another path; the same bytes in many
slices, with every table in global memory, with the locate heaps in global memory, on an index built through the merge path and with the
sampled suffix array built on the device; the refusals."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, read_ssa, sw_lines
from tests import util
from tests import kount_model as km
from tests import mem_model as mm
from tests import pos_model as pm
from tests import sw_model as sw
from tests import swaln_model as sa
from tests import swlocal_model as sl

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "SWLOCAL_MANIFEST.json")))
EXTRA = sorted(k for k, e in MANIFEST.items() if not e["matrix"])
COMMITTED_SSA = {("genomes12.fmd", 8): "genomes12.s8.ssa", ("k3_both.fmd", 0): "k3_both.s0.ssa"}


def _run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=e)


@pytest.fixture(scope="module")
def placed(tmp_path_factory):
    """index, .ssa and .len.gz of (index, S, nolen) side by side under the names the command expects (as tests/test_gpu_sw.py)"""
    root = tmp_path_factory.mktemp("swlocal")
    made = {}

    def place(idx, S, nolen=False):
        if S is None:
            return os.path.join(GOLDEN, idx)
        key = (idx, S, nolen)
        if key not in made:
            d = root / ("%s.s%d%s" % (idx, S, ".nolen" if nolen else ""))
            d.mkdir()
            loc = str(d / idx)
            shutil.copy(os.path.join(GOLDEN, idx), loc)
            if not nolen:
                shutil.copy(os.path.join(GOLDEN, idx.split(".")[0] + ".len.gz"), loc + ".len.gz")
            if (idx, S) in COMMITTED_SSA:
                shutil.copy(os.path.join(GOLDEN, COMMITTED_SSA[(idx, S)]), loc + ".ssa")
            else:
                r = _run([CLI, "ssa", "-s%d" % S, "-o", loc + ".ssa", loc])
                assert r.returncode == 0, r.stderr.decode(errors="replace")[-1000:]
            made[key] = loc
        return made[key]
    return place


def _args(e, placed):
    return e["opts"] + [placed(e["files"][0], e["S"], e["nolen"])] + [os.path.join(GOLDEN, f) for f in e["files"][1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_matches_recorded(key, placed):
    e = MANIFEST[key]
    r = _run([CLI, "sw", "--local"] + _args(e, placed))
    if "refused" in e:   # the reference's message, nothing on stdout
        assert r.returncode == 1 and r.stdout == b"" and e["refused"].encode() in r.stderr
        return
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.count(b"\n") == e["lines"]
    assert hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", EXTRA)
def test_cli_matches_live_reference(key, placed):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    e = MANIFEST[key]
    ref = _run([util.REF_BIN, "sw"] + _args(e, placed))
    r = _run([CLI, "sw", "--local"] + _args(e, placed))
    assert r.stdout == ref.stdout
    assert r.returncode == (1 if "refused" in e else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RB3GPU_SW_SLICE": "3"}, {"RB3GPU_SW_TABLE": "1"}, {"RB3GPU_LOCATE_HEAP": "1"}, {"RB3GPU_SW_TABLE": "128", "RB3GPU_SW_SLICE": "50", "RB3GPU_LOCATE_HEAP": "2"}],
                         ids=["slice3", "table1", "heap1", "table128-slice50-heap2"])
@pytest.mark.parametrize("key", ["-s8 -p3 genomes12.fmd sw_reads.fa", "-s0 -p50 genomes12.fmd sw_reads.fa", "-s8 -N200 -m10 -k3 -p2 genomes12.fmd mem_iupac.fa",
                                 "-s3 -L -m5 -k2 -p5 longruns.fmd sw_runs.txt"])
def test_cli_slices_and_global_memory_change_nothing(key, env, placed):
    e = MANIFEST[key]
    r = _run([CLI, "sw", "--local"] + _args(e, placed), env)
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
def test_cli_refusals(tmp_path, placed):
    idx, q = placed("genomes12.fmd", 8), os.path.join(GOLDEN, "mem_iupac.fa")
    for bad in (["--local", "-e"], ["--local", "--all-e2e"], ["--local", "-g2"], ["--local", "-j12"], ["--local", "-k5", "-j6"], ["--local", "-N0"], ["--local", "-k0"],
                ["--local", "-a5"], ["--local", "--cov"], ["--local", "--old-mem"]):
        r = _run([CLI, "sw"] + bad + [idx, q])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1, bad
    r = _run([CLI, "sw", "--local", str(tmp_path / "missing.fmd"), q])
    assert r.returncode == 1 and r.stdout == b"" and b"failed to load index" in r.stderr
    for opts, S, nolen in ((["-p3"], None, False), (["-p3"], 8, True), (["--no-ssa", "-p3"], 8, False)):   # -p needs both files
        r = _run([CLI, "sw", "--local"] + opts + [placed("genomes12.fmd", S, nolen), q])
        assert r.returncode == 1 and r.stdout == b"" and b"ERROR: failed to load suffix array samples or sequence names/lengths" in r.stderr, opts
    r = _run([CLI, "sw", "--local", "-j1", "-k5", "-j5", "-t3", "-C", "1k", "-M", "-b", "-y2", idx, q])   # -j up to the end length, -t -C -M -b -y: accepted, nothing changes
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == MANIFEST["-s8 -k5 genomes12.fmd mem_iupac.fa"]["md5"]
    r = _run([CLI, "sw", "--local", os.path.join(GOLDEN, "k2_fwd.fmd"), q])
    assert r.returncode == 1 and r.stdout == b"" and b"ERROR: BWT doesn't contain both strands" in r.stderr


def _random_index(seed, n_genomes=4, length=2500):
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, length)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(n_genomes - 1)]
    recs.append(np.concatenate([g0[100:400], np.full(3, 5, dtype=np.uint8), g0[:200]]))   # N inside, a repeat
    return rng, g0, recs


def _steps_bytes(steps):
    return bytes(op << 4 | b for op, b in steps)


def _check(h, ix, queries, opt, max_pos, stats=None):
    """the engine's hit is the model's, byte for byte, with its place on the query; its positions are the first n of what locate gives for the interval"""
    st = {} if stats is None else stats
    got = h.sw_local(queries, max_pos=max_pos, stats=st, **opt)
    assert len(got) == len(queries)
    n_hits = n_node = n_cut = 0
    for q, mine in zip(queries, got):
        w = sl.align(ix, q, opt)
        n_node, n_cut = n_node + sl.align.last["n_node"], n_cut + sl.align.last["n_cut"]
        if w is None:
            assert mine == []
            continue
        assert len(mine) == 1
        x = mine[0]
        assert (x["lo"], x["hi"], x["score"], x["steps"], x["qoff0"], x["n_qoff"]) == (w["lo"], w["hi"], w["score"], _steps_bytes(w["steps"]), w["qoff0"], w["n_qoff"])
        assert (x["qlen"], x["rlen"]) == sa.lens_of(w["steps"]) and x["qoff0"] + x["qlen"] <= len(q)
        if max_pos is not None:
            n = sl.n_positions(w, max_pos)
            off, pos = h.locate([x["lo"]], [x["hi"]], max(max_pos, 1))
            assert len(x["pos"]) == n and np.array_equal(x["pos"], pos[off[0]:off[0] + n])
        else:
            assert len(x["pos"]) == 0
        n_hits += 1
    assert st["n_hits"] == n_hits and st["n_nodes"] == n_node
    return got, n_cut


@pytest.mark.gpu
def test_api_matches_model():
    rng, g0, recs = _random_index(5)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(util.make_text(recs)))
        h.keep_ssa(3)
        ix = sw.BwtIndex(h.export_plain())
        twelve = g0[1000:1012]
        queries = [np.zeros(0, dtype=np.uint8), g0[:1], g0[5:7], g0[40:51], g0[40:52],              # lengths 0, 1, 2, end_len, end_len + 1
                   np.concatenate([twelve[:6], twelve[7:]]),                                        # a 12-mer with one deleted base
                   np.full(40, 5, dtype=np.uint8),                                                  # only N: a chain of A
                   util.mutate(rng, g0[300:340], 0.05), util.revcomp(util.mutate(rng, g0[700:745], 0.04)),
                   np.concatenate([g0[1500:1520], g0[1523:1545]]), np.concatenate([g0[1700:1720], util.random_genome(rng, 2), g0[1720:1742]]),
                   np.concatenate([util.random_genome(rng, 8), g0[2000:2030], util.random_genome(rng, 6)]),   # a local hit in the middle
                   np.concatenate([g0[:20], np.full(1, 5, dtype=np.uint8), g0[21:44]]), util.random_genome(rng, 40)]
        total, ops, cuts = 0, set(), 0
        for opt in (dict(n_best=1, end_len=11, min_sc=1), dict(n_best=3, end_len=11, min_sc=5), dict(n_best=200, end_len=11, min_sc=10), dict(n_best=25, end_len=11),
                    dict(n_best=3, end_len=2, min_sc=5), dict(n_best=25, end_len=3, min_sc=10), dict(n_best=7, end_len=2, match=2, mis=4, gap_open=4, gap_ext=1, min_sc=8)):
            for max_pos in (None, 0, 3):
                st = {}
                got, n_cut = _check(h, ix, queries, opt, max_pos, st)
                assert got[0] == [] and st["n_slices"] == 1 and st["n_edges"] >= st["n_nodes"] - len(queries)
                if opt["n_best"] > 32:
                    assert st["n_tier2"] > 0           # (the rows of -N200 and their table live in global memory)
                total += st["n_hits"]
                cuts += n_cut
                ops |= set(b >> 4 for mine in got for x in mine for b in x["steps"])
        assert total > 100 and ops == {0, 1, 2, 3} and cuts > 0
        # the same bytes in slices of 3 queries / of one, with every table in global memory, with the locate heaps in global memory
        opt = dict(n_best=3, end_len=2, min_sc=5)
        base, _ = _check(h, ix, queries, opt, 3)
        flat = lambda hits: [[(x["lo"], x["hi"], x["score"], x["steps"], x["qoff0"], x["n_qoff"], x["pos"].tobytes()) for x in m] for m in hits]
        for key, v, n_slices in (("sw_slice", 3, (len(queries) + 2) // 3), ("sw_table", 1, (len(queries) + 2) // 3), ("locate_heap", 1, (len(queries) + 2) // 3), ("sw_slice", 1, len(queries))):
            h.tune(key, v)
            st, lst = {}, {}
            again = h.sw_local(queries, max_pos=3, stats=st, locate_stats=lst, **opt)
            assert flat(again) == flat(base) and st["n_slices"] == n_slices, key
            if key != "sw_slice" or v == 1:
                assert st["n_tier2"] == len(queries)
            if key == "locate_heap":
                assert lst["n_tier2"] > 0
    finally:
        h.close()


def _text(strings):
    parts = []
    for s in strings:
        parts += [np.asarray(s, dtype=np.uint8), np.zeros(1, dtype=np.uint8)]
    return np.concatenate(parts)


@pytest.mark.gpu
def test_merged_index_and_device_made_ssa_give_the_same_bytes():
    """the twelve genomes: the index loaded from its plain BWT with the .ssa of the file answers with the recorded bytes through the Python formatter; the
    sampled suffix array built on the device gives the same lines; and so does the index of the first six genomes built through the merge path"""
    e = MANIFEST["-s8 -p3 genomes12.fmd sw_reads.fa"]
    qs = mm.read_queries(os.path.join(GOLDEN, "sw_reads.fa"))
    names, lengths = pm.read_len_gz(os.path.join(GOLDEN, "genomes12.len.gz"))
    seqs = [s for _, s in qs]
    whole = Rb3Gpu(verbose=1)
    try:
        whole.from_plain(km.golden_plain(GOLDEN, "genomes12.fmd", CLI))
        whole.set_ssa(*read_ssa(os.path.join(GOLDEN, "genomes12.s8.ssa")))
        hits = whole.sw_local(seqs, max_pos=3)
        assert hashlib.md5(sw_lines(seqs, hits, [n for n, _ in qs], seq_names=names, lengths=lengths)).hexdigest() == e["md5"]
        whole.keep_ssa(8)
        again = whole.sw_local(seqs, max_pos=3)
        assert sw_lines(seqs, again, seq_names=names, lengths=lengths) == sw_lines(seqs, hits, seq_names=names, lengths=lengths)
        plain = whole.sw_local(seqs)
        assert hashlib.md5(sw_lines(seqs, plain, [n for n, _ in qs], unmapped=True)).hexdigest() != e["md5"]
        assert sw_lines(seqs, plain, [n for n, _ in qs]).count(b"\n") == e["lines"]
    finally:
        whole.close()
    a = km.golden_plain(GOLDEN, "genomes12_first6.fmd", CLI)
    h, other = Rb3Gpu(verbose=1), Rb3Gpu(verbose=1)
    try:
        recs = [s for s in km.strings_of(a)]
        half = len(recs) // 2
        h.from_plain(host.build_bwt(_text(recs[:half])))
        h.merge_plain(host.build_bwt(_text(recs[half:])))
        other.from_plain(a)
        h.keep_ssa(4)
        other.keep_ssa(4)
        for n_best in (5, 25):
            x, y = h.sw_local(seqs, n_best=n_best, max_pos=2), other.sw_local(seqs, n_best=n_best, max_pos=2)
            assert sw_lines(seqs, x) == sw_lines(seqs, y) and sum(len(m) for m in x) > 100
        e6 = MANIFEST["-N5 genomes12_first6.fmd sw_reads.fa"]
        none = other.sw_local(seqs, n_best=5)
        assert hashlib.md5(sw_lines(seqs, none, [n for n, _ in qs])).hexdigest() == e6["md5"]
    finally:
        h.close()
        other.close()


@pytest.mark.gpu
def test_api_refusals():
    h, fwd, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(km.golden_plain(GOLDEN, "k4_readme.fmd", CLI))
        fwd.from_plain(km.golden_plain(GOLDEN, "k2_fwd.fmd", CLI))
        for bad in (dict(n_best=0), dict(end_len=0), dict(n_best=1 << 24), dict(n_best=(1 << 23) + 1)):   # the last: more than 512 nodes of n_best cells are 2^32 cells and more
            with pytest.raises(Rb3GpuError) as e:
                h.sw_local(["ACGTTGCATTAGGCAT" * 32], **bad)
            assert e.value.code == -3, bad
        for x in (fwd, empty):
            with pytest.raises(Rb3GpuError) as e:
                x.sw_local(["ACGTACGT"])
            assert e.value.code == -5
        with pytest.raises(Rb3GpuError) as e:            # positions without a sampled suffix array
            h.sw_local(["ACGTACGT"], max_pos=0)
        assert e.value.code == -5
        g = host.dawg_batch([0, 4], mm.nt6(b"ACGT"))
        for key, v in (("pre", np.full_like(g["pre"], 7)), ("pre_off", g["pre_off"][::-1].copy()), ("node_off", np.array([0, 40], dtype=np.int64))):   # not a graph of the query
            with pytest.raises((Rb3GpuError, ValueError)):
                h.sw_local(["ACGT"], dawg=dict(g, **{key: v}))
        assert h.sw_local([]) == [] and h.sw_local(["", ""]) == [[], []]
        got = h.sw_local(["ACG", "", "ACGTA"], min_sc=1, end_len=1)
        assert got[1] == [] and len(got) == 3
    finally:
        for x in (h, fwd, empty):
            x.close()
