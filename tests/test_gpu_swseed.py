"""sw --prefilter on the GPU: the CLI against the reference's recorded answers with -j above the end length
(tests/golden/SWSEED_MANIFEST.json: the reference's options, with `--prefilter`, and `--local` where the reference runs its default mode,
in front) and, outside the regular matrix, the live reference binary byte for byte; the same bytes with walkers of 7 window starts in
launches of 3; `--prefilter` where the reference does not filter against the existing goldens; Rb3Gpu.seed_present against the model
(tests/seed_model.py) at the query shapes and chunk sizes where the kernel can go wrong, with the model's step count; the alignments of
the queries that pass against the alignment models; the refusals."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError
from tests import util
from tests import kount_model as km
from tests import mem_model as mm
from tests import seed_model as sm
from tests import sw_model as sw
from tests import swaln_model as sa
from tests import swlocal_model as sl

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "SWSEED_MANIFEST.json")))
EXTRA = sorted(k for k, e in MANIFEST.items() if not e["matrix"])
COMMITTED_SSA = {("genomes12.fmd", 8): "genomes12.s8.ssa", ("k3_both.fmd", 0): "k3_both.s0.ssa"}
SMALL = {"RB3GPU_SEED_CHUNK": "7", "RB3GPU_SEED_SLICE": "3", "RB3GPU_SW_SLICE": "3"}


def _run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=e)


@pytest.fixture(scope="module")
def placed(tmp_path_factory):
    """index, .ssa and .len.gz of (index, S) side by side under the names the command expects (as tests/test_gpu_sw.py)"""
    root = tmp_path_factory.mktemp("swseed")
    made = {}

    def place(idx, S):
        if S is None:
            return os.path.join(GOLDEN, idx)
        if (idx, S) not in made:
            d = root / ("%s.s%d" % (idx, S))
            d.mkdir()
            loc = str(d / idx)
            shutil.copy(os.path.join(GOLDEN, idx), loc)
            shutil.copy(os.path.join(GOLDEN, idx.split(".")[0] + ".len.gz"), loc + ".len.gz")
            if (idx, S) in COMMITTED_SSA:
                shutil.copy(os.path.join(GOLDEN, COMMITTED_SSA[(idx, S)]), loc + ".ssa")
            else:
                r = _run([CLI, "ssa", "-s%d" % S, "-o", loc + ".ssa", loc])
                assert r.returncode == 0, r.stderr.decode(errors="replace")[-1000:]
            made[(idx, S)] = loc
        return made[(idx, S)]
    return place


def _mode(opts):
    """this command's switches in front of the reference's options"""
    e2e = any(o in ("-e", "--all-e2e") or o.startswith("-g") for o in opts)
    return ["--prefilter"] + ([] if e2e else ["--local"])


def _args(e, placed, opts=None):
    return (e["opts"] if opts is None else opts) + [placed(e["files"][0], e["S"])] + [os.path.join(GOLDEN, f) for f in e["files"][1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_matches_recorded(key, placed):
    e = MANIFEST[key]
    r = _run([CLI, "sw"] + _mode(e["opts"]) + _args(e, placed))
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
    r = _run([CLI, "sw"] + _mode(e["opts"]) + _args(e, placed))
    assert r.returncode == 0 and r.stdout == ref.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["-s8 -e -j30 genomes12.fmd sw_reads.fa", "-s8 -j40 genomes12.fmd sw_reads.fa", "-s8 -g2 -b -j30 genomes12.fmd sw_reads.fa",
                                 "-s8 -e -j30 genomes12.fmd mem_mutated.fa.gz"])
def test_cli_small_chunks_and_slices_change_nothing(key, placed):
    e = MANIFEST[key]
    r = _run([CLI, "sw"] + _mode(e["opts"]) + _args(e, placed), dict(SMALL, RB3_VERBOSE="3"))
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == e["md5"]
    assert b"the pre-filter: " in r.stderr and b"the seed kernel" in r.stderr     # the summary of RB3_VERBOSE=3 names the filter


@pytest.mark.gpu
def test_cli_prefilter_is_a_no_op_where_the_reference_does_not_filter(placed):
    """--prefilter without -j, and with -j at or below the end length: the bytes of the command without it (the existing goldens)"""
    e2e = json.load(open(os.path.join(GOLDEN, "SW_MANIFEST.json")))
    loc = json.load(open(os.path.join(GOLDEN, "SWLOCAL_MANIFEST.json")))
    idx, q = placed("genomes12.fmd", 8), os.path.join(GOLDEN, "sw_reads.fa")
    for man, mode, key, opts in ((e2e, [], "-s8 -e genomes12.fmd sw_reads.fa", ["-e"]), (e2e, [], "-s8 -e genomes12.fmd sw_reads.fa", ["-e", "-j1"]),
                                 (e2e, [], "-s8 -e -k5 genomes12.fmd sw_reads.fa", ["-e", "-k5", "-j5"]), (e2e, [], "-s8 -e -u genomes12.fmd sw_reads.fa", ["-j40", "-e", "-u", "-j1"]),
                                 (e2e, [], "-s8 -g1 -b genomes12.fmd sw_reads.fa", ["-g1", "-b", "-j1"]),
                                 (loc, ["--local"], "-s8 genomes12.fmd sw_reads.fa", []), (loc, ["--local"], "-s8 genomes12.fmd sw_reads.fa", ["-j11"]),
                                 (loc, ["--local"], "-s8 -k5 genomes12.fmd sw_reads.fa", ["-k5", "-j5"]), (loc, ["--local"], "-s8 -u genomes12.fmd sw_reads.fa", ["-u", "-j3"])):
        r = _run([CLI, "sw", "--prefilter"] + mode + opts + [idx, q])
        assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == man[key]["md5"], opts


def _random_index(seed):
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, 2500)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(3)]
    recs.append(np.concatenate([g0[100:160], np.full(3, 5, dtype=np.uint8), g0[:50]]))   # NNN inside
    return rng, g0, recs


def _foreign(rng, ix, n, m):
    """n random symbols without a stretch of m that occurs (m >= 12: at 2 every pair of A, C, G, T occurs)"""
    while True:
        s = util.random_genome(rng, n)
        if m < 12 or not sm.present(ix, s, m)[0]:
            return s


def _queries(rng, ix, g0, m):
    if m >= 12:
        absent_m = _foreign(rng, ix, m, m)
    else:                                                 # a pair that is not indexed: one with an N, since every pair of A, C, G, T is
        absent_m = next(np.array([a, b], dtype=np.uint8) for a in range(1, 6) for b in range(1, 6) if not sm.present(ix, [a, b], 2)[0])
    long_foreign = _foreign(rng, ix, 5000, m)
    planted = long_foreign.copy()
    at = 2048 - min(3, m - 1)                             # the seed's window starts in one chunk of 7, 64 or 2048 starts and the seed ends in the next
    planted[at:at + m] = g0[700:700 + m]
    while True:                                           # a seed at the very start only (from m = 12 on: at 2 every pair occurs)
        first = np.concatenate([g0[500:500 + m], _foreign(rng, ix, 60, m)])
        if m < 12 or not sm.present(ix, first[1:], m)[0]:
            break
    while True:                                           # ... at the very end only
        last = np.concatenate([_foreign(rng, ix, 60, m), g0[900:900 + m]])
        if m < 12 or not sm.present(ix, last[:-1], m)[0]:
            break
    qs = [np.zeros(0, dtype=np.uint8), g0[300:300 + m - 1], g0[100:100 + m], util.revcomp(g0[100:100 + m]), absent_m,
          first, last,
          np.full(m, 5, dtype=np.uint8), np.full(2 * m + 1, 5, dtype=np.uint8),              # only N: NN occurs in the indexed NNN, twelve N do not
          np.concatenate([g0[2000:2000 + m - 1], np.full(1, 5, dtype=np.uint8), g0[2000 + m:2000 + 2 * m - 1]]),   # an N that is not indexed there
          long_foreign, planted, util.mutate(rng, g0[1200:1290], 0.1), g0[1500:1580]]
    return qs


@pytest.mark.gpu
def test_api_matches_model():
    rng, g0, recs = _random_index(7)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(util.make_text(recs)))
        ix = sw.BwtIndex(h.export_plain())
        for m in (2, 12, 31):
            qs = _queries(rng, ix, g0, m)
            want = [sm.present(ix, q, m) for q in qs]
            flags = np.array([p for p, _ in want], dtype=bool)
            assert flags[2] and flags[3] and not flags[0] and not flags[1] and flags[5] and flags[6] and flags[11]
            if m >= 12:
                assert not flags[4] and not flags[7] and not flags[10] and not flags[9]
                assert not sm.present(ix, qs[5][1:], m)[0] and not sm.present(ix, qs[6][:-1], m)[0]     # the one seed is at the very start / the very end
            else:
                assert flags[7] and not flags[4]                                     # NN against the indexed NNN; a pair that is not there
            st = {}
            got = h.seed_present(qs, m, chunk=1 << 20, stats=st)                     # one walker per query: the steps are the model's
            assert got.dtype == np.bool_ and np.array_equal(got, flags)
            assert st["n_steps"] == sum(s for _, s in want) and st["n_present"] == int(flags.sum()) and st["n_queries"] == len(qs)
            assert st["n_walkers"] == sum(1 for q in qs if len(q) >= m) and st["n_slices"] == 1
            for chunk in (7, 64, None):
                st = {}
                assert np.array_equal(h.seed_present(qs, m, chunk=chunk, stats=st), flags), (m, chunk)
                c = 2048 if chunk is None else chunk
                assert st["n_walkers"] == sum((len(q) - m + 1 + c - 1) // c for q in qs if len(q) >= m) and st["n_present"] == int(flags.sum())
            for chunk in (7, 64):                                                    # launches of three walkers
                h.tune("seed_slice", 3)
                st = {}
                assert np.array_equal(h.seed_present(qs, m, chunk=chunk, stats=st), flags), (m, chunk)
                assert st["n_slices"] == (st["n_walkers"] + 2) // 3
                h.tune("seed_slice", 0)
            h.tune("seed_chunk", 5)                                                  # the chunk of a call that names none
            st = {}
            assert np.array_equal(h.seed_present(qs, m, stats=st), flags) and st["n_walkers"] == sum((len(q) - m + 5) // 5 for q in qs if len(q) >= m)
            h.tune("seed_chunk", 0)
        assert h.seed_present([], 12).size == 0 and not h.seed_present(["", "ACGT"], 12).any()
        assert h.seed_present([util.sym_str(g0[:40])], 31).all()                      # characters as for suffix
    finally:
        h.close()


def _steps_bytes(steps):
    return bytes(op << 4 | b for op, b in steps)


@pytest.mark.gpu
def test_alignments_of_the_queries_that_pass_match_the_models():
    rng, g0, recs = _random_index(9)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(util.make_text(recs)))
        ix = sw.BwtIndex(h.export_plain())
        qs = [util.mutate(rng, g0[a:a + n], r) for a, n, r in ((100, 60, 0.03), (400, 45, 0.2), (800, 70, 0.1), (1200, 50, 0.3), (1500, 40, 0.0), (1700, 64, 0.15))]
        qs += [util.random_genome(rng, 50), np.zeros(0, dtype=np.uint8), util.revcomp(util.mutate(rng, g0[2000:2080], 0.05)), g0[:11]]
        flags = h.seed_present(qs, 20)
        assert np.array_equal(flags, [bool(sm.present(ix, q, 20)[0]) for q in qs]) and 2 <= int(flags.sum()) <= len(qs) - 3
        passing = [q for q, f in zip(qs, flags) if f]
        opt = dict(n_best=5, end_len=1, min_sc=20)
        for q, mine in zip(passing, h.sw_e2e(passing, **opt)):
            want = sa.align(ix, q, opt)
            assert [(x["lo"], x["hi"], x["score"], x["steps"]) for x in mine] == [(x["lo"], x["hi"], x["score"], _steps_bytes(x["steps"])) for x in want]
        opt = dict(n_best=5, end_len=11, min_sc=20)
        n = 0
        for q, mine in zip(passing, h.sw_local(passing, **opt)):
            w = sl.align(ix, q, opt)
            assert (mine == []) == (w is None)
            if w is not None:
                x = mine[0]
                assert (x["lo"], x["hi"], x["score"], x["steps"], x["qoff0"], x["n_qoff"]) == (w["lo"], w["hi"], w["score"], _steps_bytes(w["steps"]), w["qoff0"], w["n_qoff"])
                n += 1
        assert n >= 2
    finally:
        h.close()


@pytest.mark.gpu
def test_refusals_and_one_strand(placed):
    h, fwd, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(km.golden_plain(GOLDEN, "k4_readme.fmd", CLI))
        plain = km.golden_plain(GOLDEN, "k2_fwd.fmd", CLI)
        fwd.from_plain(plain)
        for bad in (1, 0, -3):
            with pytest.raises(Rb3GpuError) as e:
                h.seed_present(["ACGTACGT"], bad)
            assert e.value.code == -3, bad
        with pytest.raises(Rb3GpuError) as e:
            empty.seed_present(["ACGTACGT"], 4)
        assert e.value.code == -5
        ix = sw.BwtIndex(plain)                               # a forward-only index answers through the API ...
        strings = km.strings_of(plain)
        qs = [mm.nt6(x) for x in (b"AGG", b"AGC", b"CCT", b"GCT", b"AG", b"GG", b"TTAGCA", b"ACGT", b"")]   # CCT, GCT: the other strand, which is not indexed
        seen = set()
        for m in (2, 3):
            got = fwd.seed_present(qs, m).tolist()
            assert got == [bool(sm.present(ix, q, m)[0]) for q in qs] == [bool(sm.brute(strings, q, m)) for q in qs]
            seen |= set(got)
            assert got[0] and got[1] and not got[2]
        assert seen == {True, False}
    finally:
        for x in (h, fwd, empty):
            x.close()
    q = os.path.join(GOLDEN, "mem_iupac.fa")
    for mode in (["-e"], ["--local"]):                        # ... while the command refuses it with the reference's message
        r = _run([CLI, "sw", "--prefilter", "-j30"] + mode + [os.path.join(GOLDEN, "k2_fwd.fmd"), q])
        assert r.returncode == 1 and r.stdout == b"" and b"ERROR: BWT doesn't contain both strands" in r.stderr
    idx = placed("genomes12.fmd", 8)
    for bad in (["-e", "-j2"], ["--local", "-j12"]):          # without --prefilter: refused as before
        r = _run([CLI, "sw"] + bad + [idx, q])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1, bad
