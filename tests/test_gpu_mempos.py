"""mem -p on the GPU: the CLI against the reference's recorded answers (tests/golden/MEMPOS_MANIFEST.json: three sample rates, capped and
uncapped lines, large intervals of identical strings) and the live reference where it is built; Rb3Gpu.locate against the string model
(tests/pos_model.py); the same bytes whatever the heap tier, the slices, the walkers' chunk and the way the sampled suffix array reached
the device; an index built through the merge path; the refusals around the two side files."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, mem_lines, read_ssa
from tests import util
from tests import kount_model as km
from tests import mem_model as mm
from tests import pos_model as pm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MEMPOS_MANIFEST.json")))
LIVE = sorted(k for k, e in MANIFEST.items() if e["S"] == 3 and e["lines"] <= 1000)
MSG = b"ERROR: failed to load suffix array samples or sequence names/lengths\n"


def _run(args, env=None, timeout=600):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """index, .ssa and .len.gz of (index, S) side by side under the names the command expects; the .ssa is the reference-written golden file
    where there is one, else what `ropebwt3-amd ssa` writes (its bytes are pinned by the tests of ssa)"""
    root = tmp_path_factory.mktemp("mempos")
    done = {}

    def get(idx, S):
        if (idx, S) not in done:
            d = root / ("%s.s%d" % (idx, S))
            d.mkdir()
            loc = str(d / idx)
            shutil.copy(os.path.join(GOLDEN, idx), loc)
            shutil.copy(os.path.join(GOLDEN, idx.split(".")[0] + ".len.gz"), loc + ".len.gz")
            gold = [e["ssa"] for e in MANIFEST.values() if e["files"][0] == idx and e["S"] == S and e["ssa"]]
            if gold:
                shutil.copy(os.path.join(GOLDEN, gold[0]), loc + ".ssa")
            else:
                r = _run([CLI, "ssa", "-s%d" % S, "-o", loc + ".ssa", loc])
                assert r.returncode == 0, r.stderr.decode(errors="replace")[-1000:]
            done[(idx, S)] = loc
        return done[(idx, S)]
    return get


def _args(e, loc):
    return e["opts"] + [loc] + [os.path.join(GOLDEN, f) for f in e["files"][1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_matches_recorded(key, staged):
    e = MANIFEST[key]
    r = _run([CLI, "mem"] + _args(e, staged(e["files"][0], e["S"])))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    print(key, r.stdout.count(b"\n"), hashlib.md5(r.stdout).hexdigest())
    assert r.stdout.count(b"\n") == e["lines"]
    assert hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", LIVE)
def test_cli_matches_live_reference(key, staged):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    e = MANIFEST[key]
    loc = staged(e["files"][0], e["S"])
    ref = _run([util.REF_BIN, "mem"] + _args(e, loc))
    r = _run([CLI, "mem"] + _args(e, loc))
    assert r.returncode == 0 and r.stdout == ref.stdout


def _genomes12():
    h = Rb3Gpu(verbose=1)
    h.from_plain(km.golden_plain(GOLDEN, "genomes12.fmd", CLI))
    return h


def _pairs(off, pos, i):
    return [(int(p["sid"]), int(p["pos"])) for p in pos[int(off[i]):int(off[i + 1])]]


@pytest.mark.gpu
def test_locate_matches_model():
    strings = [pm.as_bytes(s) for s in mm.index_strings(GOLDEN, "genomes12.fmd", CLI)]
    qs = [mm.nt6(s) for _, s in mm.read_queries(os.path.join(GOLDEN, "mem_mutated.fa.gz"))]
    h = _genomes12()
    try:
        acc = h.get_acc()
        with pytest.raises(Rb3GpuError) as e:    # no sampled suffix array yet
            h.locate([acc[1]], [acc[1] + 1], 5)
        assert e.value.code == -5
        with pytest.raises(Rb3GpuError) as e:
            h.mem(qs[:1], 19, 1, max_pos=5)
        assert e.value.code == -5
        assert h.ssa_info() is None
        h.set_ssa(*read_ssa(os.path.join(GOLDEN, "genomes12.s8.ssa")))
        assert h.ssa_info()[0] == 8
        # intervals from mem records, the cap above every size: all the occurrences
        recs = h.mem(qs, 19, 1)
        st = {}
        off, pos = h.locate(recs["x0"], recs["x0"] + recs["size"], 1000, stats=st)
        assert off.size == recs.size + 1 and off[-1] == pos.size == int(recs["size"].sum()) == st["n_pairs"] and st["n_intervals"] == recs.size and st["n_pops"] > 0
        for i in range(0, recs.size, 7):
            r = recs[i]
            got = _pairs(off, pos, i)
            assert sorted(got) == sorted(pm.occurrences(strings, qs[int(r["query"])][int(r["st"]):int(r["en"])])), i
        # the cap below the size: exactly that many distinct pairs, all of them occurrences
        recs = h.mem(qs, 5, 2)
        big = recs[recs["size"] > 20][::40]
        assert big.size > 10
        for P in (1, 3, 20):
            off, pos = h.locate(big["x0"], big["x0"] + big["size"], P)
            for i, r in enumerate(big):
                got = _pairs(off, pos, i)
                assert len(got) == P and len(set(got)) == P
                assert set(got) <= pm.occurrences(strings, qs[int(r["query"])][int(r["st"]):int(r["en"])])
        # hand-made intervals
        a1, a2, a6 = int(acc[1]), int(acc[2]), int(acc[6])
        off, pos = h.locate([a1, a1 + 5, a1 + 9, a1, a1 + 77], [a1, a1 + 5, a1 + 3, a1 + 1, a1 + 78], 10)
        assert off.tolist() == [0, 0, 0, 0, 1, 2]            # empty (lo == hi, lo > hi) and two intervals of one row
        for sid, p in _pairs(off, pos, 3) + _pairs(off, pos, 4):
            assert strings[sid][p] == 1                       # a row of the A block: a suffix that starts with A
        assert h.locate([], [], 5)[1].size == 0
        assert h.locate([a1], [a2], 0)[1].size == 0
        # whole blocks with every row wanted are ONE traversal on one octet: about 2^S rank pairs per row, one after the other -- denser samples keep that short
        h.keep_ssa(2)
        st = {}
        off, pos = h.locate([a1], [a2], a2 - a1 + 5, stats=st)      # the whole of one symbol
        assert st["n_tier2"] == 1 and st["max_heap"] > 32            # far beyond the heap in LDS
        want = {(sid, i) for sid, s in enumerate(strings) for i in np.flatnonzero(np.frombuffer(s, dtype=np.uint8) == 1).tolist()}
        assert pos.size == a2 - a1 and set(_pairs(off, pos, 0)) == want
        h.keep_ssa(1)
        off, pos = h.locate([a1], [a6], a6)                   # every row that is not a sentinel's
        assert pos.size == a6 - a1 == sum(len(s) for s in strings)
        assert set(_pairs(off, pos, 0)) == {(sid, i) for sid, s in enumerate(strings) for i in range(len(s))}
        off, pos = h.locate([a1, a1], [a6, a2], 50)
        assert off.tolist() == [0, 50, 100] and len(set(_pairs(off, pos, 0))) == 50 and set(_pairs(off, pos, 1)) <= want
        for lo, hi in ((a1 - 1, a1 + 3), (0, 5), (a6 - 2, a6 + 1), (-5, a1 + 1)):
            with pytest.raises(Rb3GpuError) as e:
                h.locate([a1, lo], [a1 + 1, hi], 5)
            assert e.value.code == -3
        h.drop_ssa()
        assert h.ssa_info() is None
    finally:
        h.close()


def _same3(a, b):
    return all(np.array_equal(a[0][f], b[0][f]) for f in ("query", "x0", "size", "st", "en")) and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()


@pytest.mark.gpu
def test_independence_of_tiers_slices_chunks_and_ssa_source():
    key = "-s8 -l5 -c2 -p20 genomes12.fmd mem_mutated.fa.gz"
    e = MANIFEST[key]
    qq = mm.read_queries(os.path.join(GOLDEN, "mem_mutated.fa.gz"))
    qs, qn = [s for _, s in qq], [n for n, _ in qq]
    names, lengths = pm.read_len_gz(os.path.join(GOLDEN, "genomes12.len.gz"))
    h = _genomes12()
    try:
        h.set_ssa(*read_ssa(os.path.join(GOLDEN, "genomes12.s8.ssa")))
        ls = {}
        base = h.mem(qs, 5, 2, max_pos=20, locate_stats=ls)
        assert hashlib.md5(mem_lines(base[0], qn, positions=base[1:], seq_names=names, lengths=lengths)).hexdigest() == e["md5"]
        assert ls["n_intervals"] == base[0].size == e["lines"] and ls["n_pairs"] == base[2].size and ls["max_heap"] >= 1
        print("default heap:", ls)
        for heap in (2, 8):
            h.tune("locate_heap", heap)
            for sl in (0, 24 * 64, 1 << 20):
                h.tune("locate_slice", sl)
                ls = {}
                got = h.mem(qs, 5, 2, max_pos=20, locate_stats=ls)
                assert _same3(got, base), (heap, sl)
                assert ls["n_tier2"] > 0 and ls["max_heap"] > heap, (heap, sl, ls)
        h.tune("locate_heap", 0), h.tune("locate_slice", 0)
        h.tune("mem_slice", 3000)
        st, ls = {}, {}
        got = h.mem(qs, 5, 2, chunk=7, max_pos=20, stats=st, locate_stats=ls)
        assert _same3(got, base) and st["n_slices"] > 10 and ls["n_slices"] > 5
        h.tune("mem_slice", 0)
        h.keep_ssa(8)                     # built on the device instead of read from the file
        assert _same3(h.mem(qs, 5, 2, max_pos=20), base)
    finally:
        h.close()


@pytest.mark.gpu
def test_cli_independence(staged):
    e = MANIFEST["-s3 -l5 -c2 -p20 genomes12.fmd mem_mutated.fa.gz"]
    loc = staged("genomes12.fmd", 3)
    for env, extra in (({"RB3GPU_LOCATE_HEAP": "2"}, []), ({"RB3GPU_LOCATE_HEAP": "2", "RB3GPU_LOCATE_SLICE": "2000"}, []), ({"RB3GPU_MEM_SLICE": "1000"}, []), ({}, ["--chunk", "7"])):
        r = _run([CLI, "mem"] + extra + _args(e, loc), env=dict(os.environ, **env))
        assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == e["md5"], (env, extra)
    e = MANIFEST["-s3 -l5 -c2 -p2000 copies3000.fmd mem_mutated.fa.gz"]   # heaps beyond LDS without any tuning
    r = _run([CLI, "mem"] + _args(e, staged("copies3000.fmd", 3)))
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.gpu
def test_merged_index_keep_ssa():
    """an index of ~0.5 M symbols built in three batches through the merge path (many groups of 8192 symbols), its sampled suffix array built and kept
    on the device: every position of every match is an occurrence in the strings, all of them where the cap admits; a merge gives the array up"""
    rng = np.random.default_rng(5)
    g0 = util.random_genome(rng, 60000)
    batches = [[g0, util.mutate(rng, g0, 0.01)], [util.mutate(rng, g0, 0.02)], util.reads_from(rng, g0, 300, 150, err=0.01)]
    strings = []
    for b in batches:
        strings += [pm.as_bytes(s) for s in mm.both_strands(b)]
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(util.make_text(batches[0])))
        for b in batches[1:]:
            h.merge_plain(host.build_bwt(util.make_text(b)))
        assert h.get_tot() > 400000
        q = util.mutate(rng, g0, 0.02)
        for S in (4, 0, 9):
            h.keep_ssa(S)
            assert h.ssa_info()[0] == S
            recs, off, pos = h.mem([q], 19, 1, max_pos=4)
            assert recs.size > 500 and off.size == recs.size + 1
            for i in range(0, recs.size, 11):
                r = recs[i]
                occ = pm.occurrences(strings, q[int(r["st"]):int(r["en"])])
                got = _pairs(off, pos, i)
                assert len(occ) == r["size"] and len(got) == min(4, len(occ)) == len(set(got)) and set(got) <= occ, (S, i)
                if len(occ) <= 4:
                    assert set(got) == occ
        h.merge_plain(host.build_bwt(util.make_text([util.mutate(rng, g0, 0.03)])))
        assert h.ssa_info() is None
        with pytest.raises(Rb3GpuError) as e:
            h.mem([q], 19, 1, max_pos=4)
        assert e.value.code == -5
    finally:
        h.close()


@pytest.mark.gpu
def test_side_file_refusals(tmp_path, staged):
    src = staged("genomes12.fmd", 8)
    other = staged("k4_readme.fmd", 8)
    q = os.path.join(GOLDEN, "mem_iupac.fa")
    plain = _run([CLI, "mem", "-l31", os.path.join(GOLDEN, "genomes12.fmd"), q])
    assert plain.returncode == 0 and plain.stdout

    def case(name, ssa, lengz):
        d = tmp_path / name
        d.mkdir()
        loc = str(d / "idx.fmd")
        shutil.copy(src, loc)
        if ssa is not None:
            open(loc + ".ssa", "wb").write(ssa)
        if lengz is not None:
            open(loc + ".len.gz", "wb").write(lengz)
        return loc
    ssa, lengz = open(src + ".ssa", "rb").read(), open(src + ".len.gz", "rb").read()
    import gzip
    short = gzip.compress(b"".join(gzip.decompress(lengz).splitlines(True)[:-1]))
    bad = {"no_ssa": (None, lengz), "no_len": (ssa, None), "neither": (None, None), "magic": (b"SSX\1" + ssa[4:], lengz), "cut": (ssa[:-8], lengz),
           "other_ssa": (open(other + ".ssa", "rb").read(), lengz), "short_len": (ssa, short), "other_len": (ssa, open(other + ".len.gz", "rb").read())}
    for name, (a, b) in bad.items():
        loc = case(name, a, b)
        r = _run([CLI, "mem", "-l31", "-p", "5", loc, q])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == MSG, name
        for opts in (["-p", "0"], ["-p", "-3"], ["--gap=20", "-p", "5"]):     # no positions asked for: no files needed
            r = _run([CLI, "mem", "-l31"] + opts + [loc, q])
            assert r.returncode == 0, (name, opts)
            if "--gap=20" not in opts:
                assert r.stdout == plain.stdout, (name, opts)
        r = _run([CLI, "mem", "-l31", "--cov", "-p", "5", loc, q])           # --cov prints no positions and needs the files all the same
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == MSG, name
    good = case("good", ssa, lengz)
    r = _run([CLI, "mem", "-l31", "-p", "10", good, q])
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == MANIFEST["-s8 -l31 -p10 genomes12.fmd mem_iupac.fa"]["md5"]
    cov = _run([CLI, "mem", "-l31", "--cov", "-p", "5", good, q])
    assert cov.returncode == 0 and cov.stdout == _run([CLI, "mem", "-l31", "--cov", good, q]).stdout
