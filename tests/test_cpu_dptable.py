"""The candidate table of the dynamic program where it grows and leaves LDS, without a GPU: that the inputs of tests/dp_cases.py do to the
model's table (tests/sw_model.py, SlotTable) what each case is named for -- conditions, asserted here before any kernel is involved; that a
growth restated wrongly (a plain re-insertion) changes answers, so the comparisons of tests/test_gpu_dptable.py can fail; that the committed
fixtures are what dp_cases makes; and that the three models reproduce what the reference answered on these inputs
(tests/golden/DPTABLE_MANIFEST.json), which pins SlotTable._grow to the reference from 4 to 512 slots."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import dp_cases as dp
from tests import mem_model as mm
from tests import sw_model as sw
from tests import swaln_model as swaln
from tests import swlocal_model as swlocal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "DPTABLE_MANIFEST.json")))
RUNS = [(c.name, N) for c in dp.CASES for N in c.n_list]


def _str(x):
    return x.decode() if isinstance(x, bytes) else x


def test_fixtures_are_what_the_cases_make():
    got = mm.read_queries(os.path.join(GOLDEN, dp.GENOME_FILE))
    assert len(got) == 1 and _str(got[0][0]) == dp.GENOME_NAME and np.array_equal(mm.nt6(got[0][1]), dp.genome())
    assert dp.genome().size == dp.GENOME_LEN and set(np.unique(dp.genome())) == {1, 2, 3, 4}
    for fn, make in dp.FILES.items():
        got = mm.read_queries(os.path.join(GOLDEN, fn))
        assert [_str(n) for n, _ in got] == dp.query_names(fn)
        assert len(got) == len(make()) and all(np.array_equal(mm.nt6(s), q) for (_, s), q in zip(got, make())), fn
        assert os.path.getsize(os.path.join(GOLDEN, fn)) < 1024
    assert os.path.getsize(os.path.join(GOLDEN, dp.GENOME_FILE)) < 12 * 1024
    assert all(25 <= len(q) <= 31 for make in dp.FILES.values() for q in make())
    w = dp.windows()
    assert sum(1 for q, (s, n) in zip(w, dp.WINDOW_AT) if not np.array_equal(q, dp.genome()[s:s + n])) == 1      # the one with mutations


def test_manifest_is_complete():
    keys = set()
    for c in dp.CASES:
        for N in c.n_list:
            if c.n_list == dp.N_LIST and N not in dp.N_RECORDED:
                continue
            key = " ".join(["hapdiv" if c.kernel == "hapdiv" else "sw"] + c.args + ["-N%d" % N, c.file])
            e = MANIFEST[key]
            assert (e["case"], e["n_best"], e["file"], e["opts"]) == (c.name, N, c.file, c.args + ["-N%d" % N])
            assert e["lines"] == e["stdout"].count("\n") > 0 and hashlib.md5(e["stdout"].encode()).hexdigest() == e["md5"]
            assert "-e" in e["opts"] if c.kernel == "sw_e" else "-e" not in e["opts"]
            keys.add(key)
    assert keys == set(MANIFEST)
    for kernel in ("hapdiv", "sw_e", "sw_local"):
        ns = {MANIFEST[k]["n_best"] for k in keys if dp.BY_NAME[MANIFEST[k]["case"]].kernel == kernel}
        assert ns >= set(dp.N_RECORDED), kernel
    for k in keys:                                       # the scores of the recipe on the command line
        if MANIFEST[k]["case"] in ("hapdiv", "sw_e", "sw_local"):
            assert all(o in MANIFEST[k]["opts"] for o in ("-A2", "-B1", "-O2", "-E1", "-m10"))


@pytest.mark.parametrize("name,N", RUNS, ids=["%s-N%d" % r for r in RUNS])
def test_case_does_to_the_table_what_it_is_named_for(name, N):
    """every window or query of the case: how often its table grows, whether in the F phase, from how many slots to how many -- and that nothing
    comes near a capacity of the kernels' workspace (no case may depend on a refusal)"""
    case = dp.BY_NAME[name]
    ans, tabs = dp.run_model(case, N)                    # (Unrepresentable would be an error here: such inputs are left out)
    n_unit = len(ans)
    assert len(tabs) == n_unit > 0
    growths, in_f, start, end = case.expect[N]
    for t in tabs:
        assert t.start == start == dp._cap0(N)
        assert [a for a, _, _ in t.growths] == [start << i for i in range(len(t.growths))] and t.end() == start << len(t.growths)
        if growths is None:
            assert len(t.growths) >= 1
        else:
            assert len(t.growths) == growths and t.end() == end
            assert any(f for _, _, f in t.growths) == in_f
        assert t.end() <= dp.TAB_CAP_MIN                                        # tab_cap
        assert t.max_f_puts <= 15 * N + 64 and t.max_f_puts <= 32 * N + 64      # stack_cap (the row's n_best cells and a push per accepted put), fpar_cap
    if N in (48, 64) and growths == 1:
        assert start == dp.LDS_SLOTS and dp.n_tier2(tabs) == n_unit              # starts in LDS, must migrate in mid-window
    if N <= 32 and growths is not None and end <= dp.LDS_SLOTS:
        assert dp.n_tier2(tabs) == 0
    if N in dp.N_STAY:
        assert dp.n_tier2(tabs) == (n_unit if N == 65 else 0)


def test_the_states_the_issue_names_are_all_reached():
    seen = {}
    for name, N in RUNS:
        for t in dp.run_model(dp.BY_NAME[name], N)[1]:
            k = dp.BY_NAME[name].kernel
            seen.setdefault(k, set())
            seen[k] |= {("grow", a) for a, _, _ in t.growths} | {("f", a) for a, _, f in t.growths if f}
            if len(t.growths) >= 2:
                seen[k].add("twice")
            if t.start <= dp.LDS_SLOTS < t.end():
                seen[k].add("migrates")
            if any(f and a <= dp.LDS_SLOTS < b for a, b, f in t.growths):
                seen[k].add("migrates in F")
    for k in ("hapdiv", "sw_e", "sw_local"):
        assert {("grow", 1 << b) for b in range(2, 9)} <= seen[k] and "twice" in seen[k] and "migrates" in seen[k], k
        assert any(x[0] == "f" for x in seen[k] if isinstance(x, tuple)), k
    assert "migrates in F" in seen["hapdiv"] and "migrates in F" in seen["sw_e"] and "migrates in F" in seen["sw_local"]


def _plain(kernel, ans):
    """the answers without the model's bookkeeping"""
    if kernel == "sw_local":
        return [hit for hit, _ in ans]
    return ans


def test_a_wrongly_restated_growth_changes_answers():
    """ReinsertTable grows by putting the old entries into an empty table in slot order.  Every case of SENSITIVE answers differently with it, in
    each of the three kernels: a kernel, a model or a recording that restated the growth like that would be caught"""
    kernels = set()
    for name, N in dp.SENSITIVE:
        case = dp.BY_NAME[name]
        good, bad = dp.run_model(case, N), dp.run_model(case, N, dp.ReinsertTable)
        assert _plain(case.kernel, good[0]) != _plain(case.kernel, bad[0]), (name, N)
        kernels.add(case.kernel)
    assert kernels == {"hapdiv", "sw_e", "sw_local"}
    t = dp.ReinsertTable(8)                              # and the wrong table is a table: it finds what was put
    keys = [(10 * i + 3, 10 * i + 8) for i in range(20)]
    for lo, hi in keys:
        assert t.put(sw.Cell(lo, hi, 0))[1]
    assert len(t.growths) == 2 and all(t.find(lo, hi) is not None for lo, hi in keys) and t.count == 20


def model_stdout(case, N):
    """what the command prints for the case, from the model's answers (no suffix array: no positions)"""
    ans = dp.run_model(case, N)[0]
    qs, names = case.queries(), case.names()
    if case.kernel == "hapdiv":
        return sw.merge_lines(ans, dp.K, names)
    if case.kernel == "sw_e":
        return b"".join(swaln.paf_line(names[i], i, qs[i], h) for i, hits in enumerate(ans) for h in hits)
    return b"".join(swlocal.paf_line(names[i], i, qs[i], hit) for i, (hit, _) in enumerate(ans) if hit is not None)


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_models_reproduce_reference(key):
    e = MANIFEST[key]
    assert model_stdout(dp.BY_NAME[e["case"]], e["n_best"]).decode() == e["stdout"]
