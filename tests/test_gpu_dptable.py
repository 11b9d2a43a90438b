"""The candidate table of `hapdiv`, `sw -e` and `sw --local` (hd_merge, hd_grow, hd_tab_init, hd_tab_clear of rb3gpu_hapdiv.h) where it grows and
leaves LDS, on the inputs of tests/dp_cases.py (tests/test_cpu_dptable.py asserts what they do to the table): the Python API against the
three models at every n_best of the list, with the number of tables that ended in global memory; the same bytes with the table's LDS part cut
to 8..128 slots, so that it migrates at every size; in slices and on an index built through the merge path; the command line against the
reference's recorded answers (tests/golden/DPTABLE_MANIFEST.json) and the live reference binary.  Everything is compared exactly."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from tests import util
from tests import dp_cases as dp
from tests import swaln_model as swaln
from tests import swlocal_model as swlocal

pytestmark = pytest.mark.gpu

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "DPTABLE_MANIFEST.json")))
RUNS = [(c.name, N) for c in dp.CASES for N in c.n_list]
MAX_POS = 2
TUNE_OF = {"hapdiv": "hapdiv_table", "sw_e": "sw_table", "sw_local": "sw_table"}
LIVE = sorted(k for k, e in MANIFEST.items() if e["n_best"] == 48 or e["case"] not in ("hapdiv", "sw_e", "sw_local"))


@pytest.fixture(scope="module")
def engine():
    """the index of the genome's two strands with a sampled suffix array, on the BWT that the models walk"""
    bwt = dp.model_index()[0]
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(bwt)
        h.keep_ssa(3)
        assert np.array_equal(h.export_plain(), bwt)
        yield h
    finally:
        h.close()


def _steps_bytes(steps):
    return bytes(op << 4 | b for op, b in steps)


def _positions(h, mine, n_pos):
    """every hit's positions are the first n of what locate gives for its interval"""
    if not mine:
        return
    off, pos = h.locate([x["lo"] for x in mine], [x["hi"] for x in mine], max(MAX_POS, 1))
    for i, x in enumerate(mine):
        assert len(x["pos"]) == n_pos[i] and np.array_equal(x["pos"], pos[off[i]:off[i] + n_pos[i]])


def _run(h, case, N):
    """(what the engine answers in a form that compares, its stats): the nine numbers per window and where the windows are; the hits with their
    steps and positions"""
    st = {}
    qs, o = case.queries(), dict(case.opt, n_best=N)
    if case.kernel == "hapdiv":
        got, where = h.hapdiv(qs, dp.K, dp.W, stats=st, **o)
        return (got.tolist(), where.tolist()), st
    call = h.sw_e2e if case.kernel == "sw_e" else h.sw_local
    got = call(qs, max_pos=MAX_POS, stats=st, **o)
    keys = ("lo", "hi", "score", "steps", "qlen", "rlen") + (("qoff0", "n_qoff") if case.kernel == "sw_local" else ())
    return [[tuple(x[k] for k in keys) + (x["pos"].tobytes(),) for x in mine] for mine in got], st


def _check(h, case, N, lds_slots=dp.LDS_SLOTS):
    """the engine against the model at n_best N, and n_tier2 against the model's tables"""
    want, tabs = dp.run_model(case, N)
    qs, o, st = case.queries(), dict(case.opt, n_best=N), {}
    if case.kernel == "hapdiv":
        got, where = h.hapdiv(qs, dp.K, dp.W, stats=st, **o)
        assert where.tolist() == [list(x[:2]) for x in want] and got.tolist() == [list(x[2]) for x in want]
        assert st["n_windows"] == len(want)
    elif case.kernel == "sw_e":
        got = h.sw_e2e(qs, max_pos=MAX_POS, stats=st, **o)
        assert len(got) == len(qs)
        for q, mine, hits in zip(qs, got, want):
            assert [(x["lo"], x["hi"], x["score"], x["steps"]) for x in mine] == [(x["lo"], x["hi"], x["score"], _steps_bytes(x["steps"])) for x in hits]
            assert all((x["qlen"], x["rlen"]) == swaln.lens_of(w["steps"]) and x["qlen"] == len(q) for x, w in zip(mine, hits))
            _positions(h, mine, swaln.n_positions(hits, MAX_POS))
        assert st["n_hits"] == sum(len(hits) for hits in want) > 0
    else:
        got = h.sw_local(qs, max_pos=MAX_POS, stats=st, **o)
        assert len(got) == len(qs)
        for q, mine, (w, _) in zip(qs, got, want):
            assert len(mine) == (0 if w is None else 1)
            for x in mine:
                assert (x["lo"], x["hi"], x["score"], x["steps"], x["qoff0"], x["n_qoff"]) == (w["lo"], w["hi"], w["score"], _steps_bytes(w["steps"]), w["qoff0"], w["n_qoff"])
                assert (x["qlen"], x["rlen"]) == swaln.lens_of(w["steps"]) and x["qoff0"] + x["qlen"] <= len(q)
                _positions(h, mine, [swlocal.n_positions(w, MAX_POS)])
        assert st["n_hits"] == sum(1 for w, _ in want if w is not None) > 0 and st["n_nodes"] == sum(n for _, n in want)
    assert st["n_tier2"] == dp.n_tier2(tabs, lds_slots), (case.name, N, lds_slots)
    return st


@pytest.mark.parametrize("name,N", RUNS, ids=["%s-N%d" % r for r in RUNS])
def test_api_matches_model(engine, name, N):
    """n_tier2 makes the migration an asserted fact: none for tables that end at 256 slots or fewer, every window where one grows from 256 to 512
    (n_best 48 and 64) or starts there (65)"""
    st = _check(engine, dp.BY_NAME[name], N)
    assert st["n_slices"] == 1


# (case, n_best) -> the slots of the table's LDS part to run with; 8 and 16 for the tables that grow twice from 8 slots: either growth is the one that migrates
MIGRATIONS = [(name, N, (16, 32, 64, 128)) for name in ("hapdiv", "sw_e", "sw_local") for N in (4, 25)] + \
             [("hapdiv-twice", 2, (8, 16)), ("sw_e-twice", 2, (8, 16)), ("sw_local-twice", 25, (128,)), ("hapdiv-ties", 16, (64,)), ("sw_e-ties", 25, (128,)), ("sw_local-ties", 16, (64,))]


@pytest.mark.parametrize("name,N,sizes", MIGRATIONS, ids=["%s-N%d" % m[:2] for m in MIGRATIONS])
def test_migration_at_every_lds_size(engine, name, N, sizes):
    """the same bytes as with the whole LDS table, and as many tables in global memory as the model's tables start at or grow past the size"""
    case = dp.BY_NAME[name]
    base, _ = _run(engine, case, N)
    n_t2 = set()
    try:
        for lds in sizes:
            engine.tune(TUNE_OF[case.kernel], lds)
            st = _check(engine, case, N, lds)
            assert _run(engine, case, N)[0] == base, lds
            n_t2.add(st["n_tier2"])
    finally:
        engine.tune(TUNE_OF[case.kernel], 0)
    assert max(n_t2) > 0                                  # (at the smallest size every one of these cases has tables that leave LDS)
    assert _run(engine, case, N)[0] == base               # the tune is back


@pytest.mark.parametrize("name", ["hapdiv", "sw_e", "sw_local"])
def test_slices_and_merged_index_at_n48(engine, name):
    """the other axes of the kernels, once each where the table migrates in mid-window: many slices (a block's global table is used by one window
    after the other), and an index built in two batches through the merge path"""
    case = dp.BY_NAME[name]
    key, v = ("hapdiv_slice", 5) if case.kernel == "hapdiv" else ("sw_slice", 3)
    n_unit = len(dp.run_model(case, 48)[0])
    try:
        engine.tune(key, v)
        st = _check(engine, case, 48)
        assert st["n_slices"] == (n_unit + v - 1) // v > 1
    finally:
        engine.tune(key, 0)
    g = dp.genome()
    z = np.zeros(1, dtype=np.uint8)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(np.concatenate([g, z])))
        h.merge_plain(host.build_bwt(np.concatenate([util.revcomp(g), z])))
        assert np.array_equal(h.export_plain(), dp.model_index()[0])
        h.keep_ssa(3)
        _check(h, case, 48)
    finally:
        h.close()


def _cli(args, timeout=300):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


@pytest.fixture(scope="module")
def index_file(tmp_path_factory):
    """the genome fixture indexed by the command line"""
    fn = str(tmp_path_factory.mktemp("dptable") / "dptable_genome.fmd")
    r = _cli(["build", "-d", "-o", fn, os.path.join(GOLDEN, dp.GENOME_FILE)])
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-1000:]
    return fn


def _args(e, index_file):
    local = [] if "-e" in e["opts"] or e["cmd"] == "hapdiv" else ["--local"]
    return [e["cmd"]] + local + e["opts"] + [index_file, os.path.join(GOLDEN, e["file"])]


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_matches_recorded(key, index_file):
    e = MANIFEST[key]
    r = _cli(_args(e, index_file))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.count(b"\n") == e["lines"]
    assert hashlib.md5(r.stdout).hexdigest() == e["md5"]


@pytest.mark.parametrize("key", LIVE)
def test_cli_matches_live_reference(key, index_file):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    e = MANIFEST[key]
    ref = subprocess.run([util.REF_BIN, e["cmd"]] + e["opts"] + [index_file, os.path.join(GOLDEN, e["file"])], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = _cli(_args(e, index_file))
    assert ref.returncode == 0 and r.returncode == 0 and r.stdout == ref.stdout and len(r.stdout) > 0
