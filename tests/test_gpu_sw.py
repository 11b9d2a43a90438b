"""sw -e on the GPU: the CLI against the reference's recorded answers (tests/golden/SW_MANIFEST.json) and, outside the regular matrix, the
live reference binary byte for byte; the Python API against the model of the alignment (tests/swaln_model.py) on small random indexes at
the shapes where the kernel takes another path; the same bytes in many slices, with every table in global memory, with the locate
heaps in global memory, on an index built through the merge path and with the sampled suffix array built on the device; the refusals
and the three shapes of the PAF's position columns."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, read_ssa, sw_all_lines, sw_lines, revcomp6, SW_ALL_HEADER
from tests import util
from tests import kount_model as km
from tests import mem_model as mm
from tests import pos_model as pm
from tests import sw_model as sw
from tests import swaln_model as sa

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "SW_MANIFEST.json")))
EXTRA = sorted(k for k, e in MANIFEST.items() if not e["matrix"])
COMMITTED_SSA = {("genomes12.fmd", 8): "genomes12.s8.ssa", ("k3_both.fmd", 0): "k3_both.s0.ssa"}


def _run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=e)


@pytest.fixture(scope="module")
def placed(tmp_path_factory):
    """index, .ssa and .len.gz of (index, S, nolen) side by side under the names the command expects; the .ssa is the reference-written golden
    file where there is one, else what `ropebwt3-amd ssa` writes (its bytes are pinned by the tests of ssa)"""
    root = tmp_path_factory.mktemp("sw")
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
    r = _run([CLI, "sw"] + _args(e, placed))
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
    r = _run([CLI, "sw"] + _args(e, placed))
    assert r.stdout == ref.stdout
    assert r.returncode == (1 if "refused" in e else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RB3GPU_SW_SLICE": "3"}, {"RB3GPU_SW_TABLE": "1"}, {"RB3GPU_LOCATE_HEAP": "1"}, {"RB3GPU_SW_TABLE": "128", "RB3GPU_SW_SLICE": "50", "RB3GPU_LOCATE_HEAP": "2"}],
                         ids=["slice3", "table1", "heap1", "table128-slice50-heap2"])
@pytest.mark.parametrize("key", ["-s8 -e -p3 genomes12.fmd sw_reads.fa", "-s0 -e -p50 genomes12.fmd sw_reads.fa", "-s8 -g1 -b genomes12.fmd sw_reads.fa",
                                 "-s8 -e -L -p2000 -N3 longruns.fmd sw_runs.txt"])
def test_cli_slices_and_global_memory_change_nothing(key, env, placed):
    e = MANIFEST[key]
    r = _run([CLI, "sw"] + _args(e, placed), env)
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
def test_cli_refusals(tmp_path, placed):
    idx, q = placed("genomes12.fmd", 8), os.path.join(GOLDEN, "mem_iupac.fa")
    for bad in ([], ["-k5"], ["-u", "--seq"], ["-e", "-j2"], ["-e", "-k5", "-j6"], ["-e", "-N0"], ["-e", "-k0"], ["-k0", "-N3"], ["-e", "-a5"], ["-e", "-w5"], ["-e", "-l5"],
                ["-e", "-c2"], ["-e", "-d"], ["-e", "--gap=20"], ["-e", "--cov"], ["-e", "--old-mem"]):
        r = _run([CLI, "sw"] + bad + [idx, q])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1, bad
    assert b"local mode is not implemented: use -e" in _run([CLI, "sw", idx, q]).stderr
    r = _run([CLI, "sw", "-e", str(tmp_path / "missing.fmd"), q])
    assert r.returncode == 1 and r.stdout == b"" and b"failed to load index" in r.stderr
    for opts, S, nolen in ((["-e", "-p3"], None, False), (["-e", "-p3"], 8, True), (["--all-e2e", "-p3"], 8, False), (["-e", "--no-ssa", "-p3"], 8, False)):   # -p needs both files
        r = _run([CLI, "sw"] + opts + [placed("genomes12.fmd", S, nolen), q])
        assert r.returncode == 1 and r.stdout == b"" and b"ERROR: failed to load suffix array samples or sequence names/lengths" in r.stderr, opts
    r = _run([CLI, "sw", "-e", "-j1", "-k5", "-j5", "-t3", "-C", "1k", "-M", idx, q])          # -j up to the end length, -t -C -M: accepted, nothing changes
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == MANIFEST["-s8 -e -k5 genomes12.fmd mem_iupac.fa"]["md5"]
    r = _run([CLI, "sw", "-e", "-k5", os.path.join(GOLDEN, "k2_fwd.fmd"), q])
    assert r.returncode == 1 and r.stdout == b"" and b"ERROR: BWT doesn't contain both strands" in r.stderr
    u = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"    sw  " in u.stdout + u.stderr


@pytest.mark.gpu
def test_cli_position_columns_have_three_shapes(placed):
    """names and lengths present; the suffix array only; neither -- on the same query, columns 5-9 of the first line"""
    q = os.path.join(GOLDEN, "mem_iupac.fa")
    first = {}
    for shape, loc, opts in (("named", placed("genomes12.fmd", 8), ["-e"]), ("ssa", placed("genomes12.fmd", 8, True), ["-e"]), ("none", placed("genomes12.fmd", 8), ["-e", "--no-ssa"])):
        r = _run([CLI, "sw"] + opts + [loc, q])
        assert r.returncode == 0
        first[shape] = r.stdout.split(b"\n")[0].split(b"\t")
    names, lengths = pm.read_len_gz(os.path.join(GOLDEN, "genomes12.len.gz"))
    a, b, c = first["named"], first["ssa"], first["none"]
    assert a[:4] == b[:4] == c[:4] and a[9:] == b[9:] == c[9:]
    assert c[4:9] == [b"*", b"*", c[6], b"*", b"*"] and int(c[6]) > 0
    assert b[4] == b"+" and b[6] == b"*" and int(b[8]) - int(b[7]) == int(c[6])
    sid = int(b[5])
    assert a[4] == b"+-"[sid & 1:(sid & 1) + 1] and a[5].decode() == names[sid >> 1] and int(a[6]) == lengths[sid >> 1] and int(a[8]) - int(a[7]) == int(c[6])
    assert int(a[7]) == (int(b[7]) if sid & 1 == 0 else lengths[sid >> 1] - int(b[8]))


def _random_index(seed, n_genomes=4, length=2500):
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, length)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(n_genomes - 1)]
    recs.append(np.concatenate([g0[100:400], np.full(3, 5, dtype=np.uint8), g0[:200]]))   # N inside, a repeat
    return rng, g0, recs


def _steps_bytes(steps):
    return bytes(op << 4 | b for op, b in steps)


def _check(h, ix, queries, opt, max_pos, stats=None):
    """the engine's hits are the model's, byte for byte; their positions are the first n of what locate gives for the interval, n as rb3_sw counts it"""
    st = {} if stats is None else stats
    got = h.sw_e2e(queries, max_pos=max_pos, stats=st, **opt)
    assert len(got) == len(queries)
    n_hits = 0
    for q, mine in zip(queries, got):
        want = sa.align(ix, q, opt)
        assert [(x["lo"], x["hi"], x["score"], x["steps"]) for x in mine] == [(x["lo"], x["hi"], x["score"], _steps_bytes(x["steps"])) for x in want]
        for x, w in zip(mine, want):
            assert (x["qlen"], x["rlen"]) == sa.lens_of(w["steps"]) and x["qlen"] == len(q)
        if max_pos is not None and mine:
            n_pos = sa.n_positions(want, max_pos)
            cap = max(max_pos, 1)
            off, pos = h.locate([x["lo"] for x in mine], [x["hi"] for x in mine], cap)
            for i, x in enumerate(mine):
                assert len(x["pos"]) == n_pos[i] and np.array_equal(x["pos"], pos[off[i]:off[i] + n_pos[i]])
        else:
            assert all(len(x["pos"]) == 0 for x in mine)
        n_hits += len(mine)
    assert st["n_hits"] == n_hits
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_api_matches_model(seed):
    rng, g0, recs = _random_index(seed)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(util.make_text(recs)))
        h.keep_ssa(3)
        ix = sw.BwtIndex(h.export_plain())
        twelve = g0[1000:1012]
        queries = [g0[:1], g0[5:7], g0[40:45], g0[40:46],                                   # lengths 1, 2, end_len (5 below), end_len + 1
                   np.full(40, 5, dtype=np.uint8),                                             # only N
                   np.concatenate([twelve[:6], twelve[7:]]),                                   # a 12-mer with one deleted base
                   np.zeros(0, dtype=np.uint8),                                                # an empty query between two others
                   util.mutate(rng, g0[300:420], 0.03), util.revcomp(util.mutate(rng, g0[700:790], 0.02)),
                   np.concatenate([g0[1500:1540], g0[1543:1600]]), np.concatenate([g0[1700:1750], util.random_genome(rng, 2), g0[1750:1800]]),
                   np.concatenate([g0[:50], np.full(1, 5, dtype=np.uint8), g0[51:120]]), util.random_genome(rng, 80)]
        total, ops = 0, set()
        for opt in (dict(n_best=25, end_len=1, min_sc=1), dict(n_best=25, end_len=5, min_sc=1), dict(n_best=1, end_len=1, min_sc=5), dict(n_best=4, end_len=11),
                    dict(n_best=25, end_len=1, min_sc=10, e2e_drop=4), dict(n_best=7, end_len=2, match=2, mis=4, gap_open=4, gap_ext=1, min_sc=8)):
            for max_pos in (None, 0, 3):
                st = {}
                got = _check(h, ix, queries, opt, max_pos, st)
                assert got[6] == [] and st["n_slices"] == 1
                total += st["n_hits"]
                ops |= set(b >> 4 for mine in got for x in mine for b in x["steps"])
        assert total > 100 and ops == {0, 1, 2, 3}
        # a 300 bp query at n_best 40: rows leave LDS; a 2 kbp exact copy.  The query is aligned from its end and a score may not fall to 0,
        # so a substitution in its last few symbols leaves no end-to-end hit at all: the last 20 stay exact
        big = [np.concatenate([util.mutate(rng, g0[900:1180], 0.02), g0[1180:1200]]), g0[200:2200], g0[:3]]
        st = {}
        got = _check(h, ix, big, dict(n_best=40, end_len=1), 2, st)
        assert len(got[0]) > 0 and got[1][0]["steps"] == bytes([0 << 4 | int(b) for b in g0[200:2200]]) and got[1][0]["score"] == 2000
        want = [(x["lo"], x["hi"], x["score"], x["steps"], x["pos"].tobytes()) for mine in got for x in mine]
        # the same bytes in slices of 3 queries / of one, with every table in global memory, with the locate heaps in global memory
        opt = dict(n_best=25, end_len=1, min_sc=1)
        base = _check(h, ix, queries, opt, 3)
        flat = lambda hits: [[(x["lo"], x["hi"], x["score"], x["steps"], x["pos"].tobytes()) for x in m] for m in hits]
        for key, v, n_slices in (("sw_slice", 3, (len(queries) + 2) // 3), ("sw_table", 1, (len(queries) + 2) // 3), ("locate_heap", 1, (len(queries) + 2) // 3), ("sw_slice", 1, len(queries))):
            h.tune(key, v)
            st, lst = {}, {}
            again = h.sw_e2e(queries, max_pos=3, stats=st, locate_stats=lst, **opt)
            assert flat(again) == flat(base) and st["n_slices"] == n_slices, key
            if key != "sw_slice" or v == 1:
                assert st["n_tier2"] == sum(1 for q in queries if len(q))
            if key == "locate_heap":
                assert lst["n_tier2"] > 0
        st = {}
        again = h.sw_e2e(big, n_best=40, end_len=1, max_pos=2, stats=st)
        assert [(x["lo"], x["hi"], x["score"], x["steps"], x["pos"].tobytes()) for mine in again for x in mine] == want and st["n_slices"] == 3
    finally:
        h.close()


def _text(strings):
    """the strings as they are (both strands are among them already), each ended by a sentinel"""
    parts = []
    for s in strings:
        parts += [np.asarray(s, dtype=np.uint8), np.zeros(1, dtype=np.uint8)]
    return np.concatenate(parts)


@pytest.mark.gpu
def test_merged_index_and_device_made_ssa_give_the_same_bytes():
    """the twelve genomes: the index loaded from its plain BWT with the .ssa of the file answers with the recorded bytes, through the Python
    formatters; the sampled suffix array built on the device gives the same hits and positions; and so does the index of the first six
    genomes built in two batches through the merge path against the one that was loaded"""
    e = MANIFEST["-s8 -e -p3 genomes12.fmd sw_reads.fa"]
    qs = mm.read_queries(os.path.join(GOLDEN, "sw_reads.fa"))
    names, lengths = pm.read_len_gz(os.path.join(GOLDEN, "genomes12.len.gz"))
    whole = Rb3Gpu(verbose=1)
    try:
        whole.from_plain(km.golden_plain(GOLDEN, "genomes12.fmd", CLI))
        whole.set_ssa(*read_ssa(os.path.join(GOLDEN, "genomes12.s8.ssa")))
        seqs = [s for _, s in qs]
        hits = whole.sw_e2e(seqs, max_pos=3)
        assert hashlib.md5(sw_lines(seqs, hits, [n for n, _ in qs], seq_names=names, lengths=lengths)).hexdigest() == e["md5"]
        whole.keep_ssa(8)
        again = whole.sw_e2e(seqs, max_pos=3)
        assert sw_lines(seqs, again, seq_names=names, lengths=lengths) == sw_lines(seqs, hits, seq_names=names, lengths=lengths)
        whole.keep_ssa(2)                  # another sample rate: other rows are sampled, so only a full listing must agree
        few = [s for s in seqs[:40]]
        x, y = whole.sw_e2e(few, max_pos=1 << 20), None
        whole.set_ssa(*read_ssa(os.path.join(GOLDEN, "genomes12.s8.ssa")))
        y = whole.sw_e2e(few, max_pos=1 << 20)
        for a, b in zip(x, y):
            assert [(h["lo"], h["steps"]) for h in a] == [(h["lo"], h["steps"]) for h in b]
            for ha, hb in zip(a, b):
                assert sorted(map(tuple, ha["pos"].tolist())) == sorted(map(tuple, hb["pos"].tolist()))
        e = MANIFEST["-s8 --all-e2e -g3 genomes12.fmd sw_reads.fa"]
        plain = whole.sw_e2e(seqs)
        assert hashlib.md5(SW_ALL_HEADER + sw_all_lines(seqs, plain, [n for n, _ in qs], max_out=3)).hexdigest() == e["md5"]
        e = MANIFEST["-s8 -g1 -b genomes12.fmd sw_reads.fa"]
        rev = whole.sw_e2e([revcomp6(mm.nt6(s)) for s in seqs])
        assert hashlib.md5(SW_ALL_HEADER + sw_all_lines(seqs, plain, [n for n, _ in qs], max_out=1, hits_rev=rev)).hexdigest() == e["md5"]
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
            x, y = h.sw_e2e(seqs, n_best=n_best, max_pos=2), other.sw_e2e(seqs, n_best=n_best, max_pos=2)
            assert sw_lines(seqs, x) == sw_lines(seqs, y) and sum(len(m) for m in x) > 100
    finally:
        h.close()
        other.close()


@pytest.mark.gpu
def test_api_refusals():
    h, fwd, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(km.golden_plain(GOLDEN, "k4_readme.fmd", CLI))
        fwd.from_plain(km.golden_plain(GOLDEN, "k2_fwd.fmd", CLI))
        for bad in (dict(n_best=0), dict(end_len=0), dict(n_best=1 << 24), dict(n_best=(1 << 23) + 1)):   # the last: 513 rows of n_best cells are 2^32 cells and more
            with pytest.raises(Rb3GpuError) as e:
                h.sw_e2e(["ACGTACGT" * 64], **bad)
            assert e.value.code == -3, bad
        for x in (fwd, empty):
            with pytest.raises(Rb3GpuError) as e:
                x.sw_e2e(["ACGTACGT"])
            assert e.value.code == -5
        with pytest.raises(Rb3GpuError) as e:            # positions without a sampled suffix array
            h.sw_e2e(["ACGTACGT"], max_pos=0)
        assert e.value.code == -5
        assert h.sw_e2e([]) == [] and h.sw_e2e(["", ""]) == [[], []]
        got = h.sw_e2e(["ACG", "", "ACGTA"], min_sc=1)
        assert got[1] == [] and len(got) == 3
    finally:
        for x in (h, fwd, empty):
            x.close()
