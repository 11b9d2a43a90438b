"""Parity of the HIP engine (through the C ABI) against the CPU oracle.  Bit-exact: this is
integer/byte work, so every comparison is array_equal."""
import os
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu


def _bwt_of(oracle, seqs, **kw):
    return oracle.bwt(util.make_text(seqs, **kw))


def test_k2_toy(engine, oracle):
    # AGG then AGC, forward only -> GC$$GGAA through the merge
    b1 = oracle.bwt(oracle.text(["AGG"], True, False))
    b2 = oracle.bwt(oracle.text(["AGC"], True, False))
    engine.from_plain(b1)
    assert util.sym_str(engine.export_plain()) == "G$GA"
    pos, acc2 = engine.mg_rank_plain(b2)
    assert list(pos) == [1, 2, 4, 6]  # chain rows 0->2->3->1 land on 1,4,6,2
    engine.merge_plain(b2)
    assert util.sym_str(engine.export_plain()) == "GC$$GGAA"
    assert list(engine.get_acc()) == [0, 2, 4, 5, 8, 8, 8]


def test_k3_toy_both_strands(engine, oracle):
    b1 = oracle.bwt(oracle.text(["AGG"]))
    b2 = oracle.bwt(oracle.text(["AGC"]))
    engine.from_plain(b1)
    engine.merge_plain(b2)
    assert util.sym_str(engine.export_plain()) == "GTCT$$G$CGGA$ACC"


@pytest.mark.parametrize("n,seed", [(1, 1), (255, 2), (256, 3), (257, 4), (8191, 5), (8192, 6), (8193, 7), (100000, 8)])
def test_from_plain_roundtrip_and_rank(engine, oracle, n, seed):
    rng = np.random.default_rng(seed)
    # a mix of random symbols and long runs so that both slot kinds appear
    parts, tot = [], 0
    while tot < n:
        if rng.random() < 0.5:
            l = int(rng.integers(1, 600))
            p = rng.integers(0, 6, size=l, dtype=np.uint8)
        else:
            l = int(rng.integers(1, 20000))
            p = np.full(l, rng.integers(0, 6), dtype=np.uint8)
        parts.append(p)
        tot += l
    b = np.concatenate(parts)[:n]
    engine.from_plain(b)
    assert engine.get_tot() == n
    assert np.array_equal(engine.export_plain(), b)
    runs = engine.export_runs()
    assert sum(l for _, l in runs) == n
    # rank at every boundary-ish offset and random offsets, incl. k = n (mrope.c:89-93)
    ks = np.unique(np.concatenate([rng.integers(0, n + 1, size=2000), np.array([0, n, n // 2]),
                                   np.arange(0, n + 1, 256)[:2000], np.clip(np.arange(0, n + 1, 8192) - 1, 0, n)]))
    ok = engine.rank1a(ks)
    occ = np.zeros((n + 1, 6), dtype=np.int64)
    for c in range(6):
        occ[1:, c] = np.cumsum(b == c)
    assert np.array_equal(ok, occ[ks])
    acc = engine.get_acc()
    assert np.array_equal(acc[1:], np.cumsum(occ[n]))


def _merge_case(engine, oracle, seqs1, seqs2, split_log2=None):
    b1 = _bwt_of(oracle, seqs1)
    b2 = _bwt_of(oracle, seqs2)
    rb, acc2 = oracle.mg_rank(b1, b2)
    want = oracle.merge(b1, b2)
    engine.from_plain(b1)
    pos, gacc2 = engine.mg_rank_plain(b2)
    assert np.array_equal(gacc2, acc2)
    assert np.array_equal(pos, rb >> 6)
    engine.merge_plain(b2)
    got = engine.export_plain()
    assert np.array_equal(got, want)
    return want


def test_merge_random_genomes(engine, oracle):
    rng = np.random.default_rng(11)
    g0 = util.random_genome(rng, 30000)
    g1 = util.mutate(rng, g0, 0.01)
    _merge_case(engine, oracle, [g0], [g1])


def test_merge_reads_with_duplicates(engine, oracle):
    rng = np.random.default_rng(12)
    g = util.random_genome(rng, 5000)
    r1 = util.reads_from(rng, g, 300, 100)
    r2 = util.reads_from(rng, g, 300, 100, err=0.01)
    r2 += r1[:20]                      # exact duplicates: ties broken by sentinel order
    r2.append(util.revcomp(r1[3]))     # reverse-complement duplicate
    _merge_case(engine, oracle, r1, r2)


def test_merge_incremental_many_rounds(engine, oracle):
    rng = np.random.default_rng(13)
    g = util.random_genome(rng, 3000)
    seqs = [util.mutate(rng, g, 0.005) for _ in range(12)]
    cur = _bwt_of(oracle, seqs[:1])
    engine.from_plain(cur)
    for s in seqs[1:]:
        b2 = _bwt_of(oracle, [s])
        cur = oracle.merge(cur, b2)
        engine.merge_plain(b2)
    assert np.array_equal(engine.export_plain(), cur)
    # the .fmd is a function of the string list only: one big batch gives the same BWT
    assert np.array_equal(cur, _bwt_of(oracle, seqs))


def test_merge_new_suffix_after_everything(engine, oracle):
    # ka == n1: the new strings sort after everything already indexed (mrope.c:89-93)
    a = np.full(300, 1, dtype=np.uint8)
    t = np.full(300, 4, dtype=np.uint8)
    n5 = np.full(50, 5, dtype=np.uint8)
    b1 = oracle.bwt(util.make_text([a], rev=False))
    b2 = oracle.bwt(util.make_text([t, n5], rev=False))
    want = oracle.merge(b1, b2)
    engine.from_plain(b1)
    engine.merge_plain(b2)
    assert np.array_equal(engine.export_plain(), want)


def test_bad_symbol_rejected(engine):
    from ropebwt3_amd import Rb3GpuError
    b = np.array([1, 2, 0, 9, 0], dtype=np.uint8)
    with pytest.raises(Rb3GpuError) as e:
        engine.from_plain(b)
    assert e.value.code == -4


@pytest.mark.parametrize("step", [16, 100, 1024])
def test_merge_with_host_walkers(engine, oracle, step):
    """rb3gpu_merge_plain_walkers: text-regular walkers from the host suffix sorter give the same pos[]"""
    from ropebwt3_amd import host
    rng = np.random.default_rng(21)
    g0 = util.random_genome(rng, 20000)
    seqs2 = [util.mutate(rng, g0, 0.002), util.mutate(rng, g0, 0.01)[:7777], g0[:50].copy(), g0.copy()] + util.reads_from(rng, g0, 30, 80)
    b1 = oracle.bwt(util.make_text([g0]))
    t2 = util.make_text(seqs2)
    b2, w = host.build_bwt_walkers(t2, step)
    assert np.array_equal(b2, oracle.bwt(t2))
    assert (w[:, 1] == -2).sum() == 2 * len(seqs2)
    want = oracle.merge(b1, b2)
    engine.from_plain(b1)
    engine.merge_plain_walkers(b2, w)
    assert np.array_equal(engine.export_plain(), want)


def test_staged_merge_with_stop_and_fixup(engine, oracle):
    """the multi-GPU protocol on one GPU: two 'ranks' own the two halves of the walker list; walkers of
    the upper half stop at the row where the lower half's territory begins and leave the value they
    arrive with, which a fix-up walker of the lower half picks up"""
    from ropebwt3_amd import host, multi
    rng = np.random.default_rng(22)
    g0 = util.random_genome(rng, 30000)
    b1 = oracle.bwt(util.make_text([g0]))
    for seqs, step in (([util.mutate(rng, g0, 0.003)], 512), ([g0[5000:9000].copy()], 256)):   # 2nd: nothing converges
        t2 = util.make_text(seqs, rev=False)
        b2, w = host.build_bwt_walkers(t2, step)
        rb, _ = oracle.mg_rank(b1, b2)
        engine.from_plain(b1)
        d = engine.dev_upload(b2)
        bounds = multi.partition(w, 2, step)
        lo_part, stop_lo, src_lo = multi.slice_plan(w, bounds, 0)
        hi_part, stop_hi, src_hi = multi.slice_plan(w, bounds, 1)
        assert stop_lo == -1 and src_lo == 1 and stop_hi == lo_part[-1, 0] and src_hi == -1
        engine.mg_begin(d, b2.size)
        val = engine.mg_walk(hi_part, stop_hi)
        assert val >= 0                  # the sentinel walker is in the upper half: an exact value always arrives
        engine.mg_walk(lo_part, -1)
        fix = np.array([[lo_part[-1, 0], val, multi.NSTEPS_INF, multi.WK_CHECK]], dtype=np.int64)
        engine.mg_walk(fix, -1)
        p, n = engine.mg_pos_ptr()
        pos = np.empty(n, dtype=np.int64)
        engine._chk(engine._lib.rb3gpu_dev_download(engine._h, pos.ctypes.data, p, n * 8), "download")
        assert np.array_equal(pos, rb >> 6)
        engine.mg_finish(commit=True)
        assert np.array_equal(engine.export_plain(), oracle.merge(b1, b2))
        engine.dev_free(d)


@pytest.mark.parametrize("seed", [31, 32, 33, 34])
def test_stress_walker_modes_vs_oracle(oracle, seed):
    """randomised inputs through every rank-phase variant (automatic split with atomic-min tentative
    records, host walker list with plain tentative records, tentative records disabled, fallback
    conditions such as tiny segments): pos[] must equal the oracle's rb[] >> 6 bit for bit"""
    import os
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(seed)
    n = int(rng.integers(60000, 200000))
    g0 = util.random_genome(rng, n)
    # index: one or several similar genomes (several => the unique-match shortcut does not apply)
    idx = [g0] + [util.mutate(rng, g0, 0.002) for _ in range(int(rng.integers(0, 3)))]
    div = float(rng.choice([0.0003, 0.001, 0.005, 0.02]))
    new = [util.mutate(rng, g0, div)]
    if seed % 2:
        new += [g0[1000:1000 + int(rng.integers(500, 40000))].copy()]          # exact duplicate of indexed text
        new += [np.concatenate([np.full(3000, 1, dtype=np.uint8), g0[:5000]])]  # long homopolymer
        new += util.reads_from(rng, g0, 50, 120, err=0.02)
    b1 = host.build_bwt(util.make_text(idx))
    t2 = util.make_text(new)
    rb, _ = oracle.mg_rank(b1, host.build_bwt(t2), 8)
    want = rb >> 6
    for split, env in ((0, {}), (6, {}), (9, {"RB3GPU_TENT": "0"}), (-1, {})):
        for k in ("RB3GPU_TENT",):
            os.environ.pop(k, None)
        os.environ.update(env)
        h = Rb3Gpu(split_log2=split, verbose=1)
        try:
            h.from_plain(b1)
            pos, _ = h.mg_rank_plain(host.build_bwt(t2))
            assert np.array_equal(pos, want), ("auto", split, env)
            for step in (32, 100, 512):
                b2, w = host.build_bwt_walkers(t2, step)
                d = h.dev_upload(b2)
                h.mg_begin(d, b2.size)
                h.mg_walk(w)          # staged API: no tentative records
                p, ln = h.mg_pos_ptr()
                got = np.empty(ln, dtype=np.int64)
                h._chk(h._lib.rb3gpu_dev_download(h._h, got.ctypes.data, p, ln * 8), "download")
                h.mg_finish(False)
                assert np.array_equal(got, want), ("staged", step, env)
                h.dev_free(d)
                got, _ = h.mg_rank_plain_walkers(b2, w)                   # single-sync path with tentative records
                assert np.array_equal(got, want), ("fast", step, env)
            st = h.stats()
            assert st["n_fallbacks"] >= 0
        finally:
            os.environ.pop("RB3GPU_TENT", None)
            h.close()
    # and the committed result of the fast path
    h = Rb3Gpu(verbose=1)
    h.from_plain(b1)
    b2, w = host.build_bwt_walkers(t2, 256)
    h.merge_plain_walkers(b2, w)
    assert np.array_equal(h.export_plain(), oracle.merge(b1, b2))
    h.close()


@pytest.mark.parametrize("seed,nrel", [(51, 2), (52, 6), (53, 12)])
def test_family_of_relatives_tentative_stretches(oracle, seed, nrel):
    """a genome merged into an index that already holds several close relatives (some identical): the
    new suffixes match k > 1 indexed suffixes for long stretches, and the walkers record tentatively
    with one stretch id per drop-out.  Bit-exact against the oracle, and far fewer LF steps than
    without tentative records (every walker stops about one segment after it started)."""
    import os
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, 40000)
    rel = [g0]
    for i in range(nrel - 1):
        src = rel[int(rng.integers(0, len(rel)))]          # a small phylogeny: mutate some earlier relative
        rel.append(src.copy() if i % 4 == 3 else util.mutate(rng, src, float(rng.choice([0.0005, 0.002, 0.01]))))
    new = [util.mutate(rng, rel[int(rng.integers(0, nrel))], 0.001), rel[-1].copy()]
    b1 = host.build_bwt(util.make_text(rel))
    t2 = util.make_text(new)
    rb, _ = oracle.mg_rank(b1, host.build_bwt(t2), 8)
    want = rb >> 6
    steps = {}
    for tent in ("1", "0"):
        os.environ["RB3GPU_TENT"] = tent
        try:
            h = Rb3Gpu(verbose=1)
            h.from_plain(b1)
            for step in (128, 384):
                b2, w = host.build_bwt_walkers(t2, step)
                got, _ = h.mg_rank_plain_walkers(b2, w)
                assert np.array_equal(got, want), (tent, step)
            pos, _ = h.mg_rank_plain(host.build_bwt(t2))   # automatic split (atomic-min records)
            assert np.array_equal(pos, want), (tent, "auto")
            st = h.stats()
            steps[tent] = st["n_lf_steps"] - 3 * want.size    # steps beyond one per row and pass
            assert st["n_fallbacks"] == 0
            h.close()
        finally:
            os.environ.pop("RB3GPU_TENT", None)
    assert steps["1"] < 0.6 * steps["0"], steps


@pytest.mark.parametrize("limit", [0, 40, 400, 4000])
def test_stretch_table_exhaustion(oracle, limit):
    """a stretch table that is (artificially) too small: walkers that cannot get their first id stay plain
    inexact walkers, walkers that run out in mid-walk poison their records; the device-side validation then
    makes the rebuild of that attempt do nothing and the host redoes the rank phase -- same index either way"""
    import os
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(71)
    g0 = util.random_genome(rng, 60000)
    rel = [g0] + [util.mutate(rng, g0, 0.003) for _ in range(9)]
    b1 = host.build_bwt(util.make_text(rel))
    b2, w = host.build_bwt_walkers(util.make_text([util.mutate(rng, g0, 0.002), rel[3].copy()]), 200)
    want = oracle.merge(b1, b2)
    try:
        h = Rb3Gpu(verbose=1, hooks=True)
        h.tune("tent_limit", limit)
        h.from_plain(b1)
        h.merge_plain_walkers(b2, w)
        st = h.stats()
        assert np.array_equal(h.export_plain(), want)
        h.merge_plain_walkers(b2, w)                       # and the handle is still fine afterwards
        assert h.get_tot() == b1.size + 2 * b2.size
        h.close()
    finally:
        pass
    print("limit", limit, "fallbacks", st["n_fallbacks"], "steps", st["n_lf_steps"])


def test_fallback_path_redoes_the_rank_phase(oracle):
    """the optimistic tentative-record pass is verified on the device; when it reports unsettled records
    the merge is redone without them (forced here through the test hook) and must give the same index"""
    import os
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(41)
    g0 = util.random_genome(rng, 50000)
    b1 = host.build_bwt(util.make_text([g0]))
    b2, w = host.build_bwt_walkers(util.make_text([util.mutate(rng, g0, 0.002)]), 256)
    want = oracle.merge(b1, b2)
    try:
        h = Rb3Gpu(verbose=1, hooks=True)
        h.tune("force_fallback", 1)
        h.from_plain(b1)
        h.merge_plain_walkers(b2, w)
        st = h.stats()
        assert st["n_fallbacks"] == 1
        assert np.array_equal(h.export_plain(), want)
        h.close()
    finally:
        pass


@pytest.mark.parametrize("seed,kind", [(61, "genomes"), (62, "reads"), (63, "runs"), (64, "tiny")])
def test_ssa_gen_vs_oracle(oracle, seed, kind):
    """sampled suffix array of the resident index (rb3gpu_ssa_gen) against the oracle's restatement of
    rb3_ssa_gen (ssa.c:17-81), for several sample rates and splitter spacings, on bit-plane and run slots"""
    import os
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(seed)
    if kind == "genomes":
        g0 = util.random_genome(rng, 60000)
        seqs = [g0] + [util.mutate(rng, g0, 0.003) for _ in range(3)]
    elif kind == "reads":
        seqs = util.reads_from(rng, util.random_genome(rng, 20000), 3000, 80, err=0.01)
    elif kind == "runs":
        seqs = [np.full(50000, 1, dtype=np.uint8), np.tile(np.array([1, 2, 3, 4], dtype=np.uint8), 3000), np.full(9000, 5, dtype=np.uint8)]
        seqs += [seqs[1].copy() for _ in range(40)]
    else:
        seqs = [np.array([1, 3, 3], dtype=np.uint8), np.array([1, 3, 2], dtype=np.uint8)]
    b = host.build_bwt(util.make_text(seqs))
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(b)
        if kind == "runs":   # through the run import too: that is how `ssa` loads an index
            runs = h.export_runs()
            h.close()
            h = Rb3Gpu(verbose=1)
            h.from_runs(runs)
        for ss in (0, 2, 5, 8, 13):
            want = oracle.ssa_gen(b, ss)
            for S in (None, 4, 7, 20):
                h.tune("ssa_split", 8 if S is None else S)
                ms, r2i, ssa = h.ssa_gen(ss)
                assert ms == want[0]
                assert np.array_equal(r2i, want[1]), (ss, S)
                assert np.array_equal(ssa, want[2]), (ss, S)
    finally:
        h.close()


def test_soak_few_cases():
    """tools/soak.py: random families (substitutions, indels, duplicates, tandem repeats, homopolymers, several
    genomes per batch, both walker modes) -- merged BWT, run export and sampled suffix array against the oracle"""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "soak.py"), "8", "5000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]


def test_soak_with_every_buffer_a_growable_range():
    """the same soak with RB3GPU_VMM=4: the slot arrays and the rebuild's scratch are ranges of reserved address space that grow in place, chunk by chunk,
    from 4 KB on (vm_ensure, round 6; by default from 64 MB on) -- and with RB3GPU_VMM=0: hipMalloc and reallocation, as in rounds 1-5"""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for v, res in (("4", "0"), ("4", "2"), ("0", "0")):   # (a reservation of 2 MB: a range that outgrows it moves, with its physical chunks, into a larger one)
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "soak.py"), "6", "5000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, RB3GPU_VMM=v, RB3GPU_VMM_RESERVE=res))
        assert r.returncode == 0, (v, res, r.stdout.decode()[-2000:])


@pytest.mark.parametrize("seed,kind", [(81, "genomes"), (82, "reads"), (83, "copies"), (84, "tiny"), (85, "runs"), (86, "family")])
def test_bwt_from_text_vs_host_sorter(oracle, seed, kind):
    """partial BWT of a batch on the GPU (rb3gpu_bwt_from_text, prefix doubling) against the host suffix sorter
    (itself pinned to the reference's libsais output): BWT bytes and the sampled inverse suffix array, every entry of which and the
    number of doubling rounds are the sorter's restatement's (tests/sort_model.py)"""
    from ropebwt3_amd import Rb3Gpu, host
    from tests import sort_model
    rng = np.random.default_rng(seed)
    if kind == "genomes":
        g0 = util.random_genome(rng, 150000)
        seqs = [g0, util.mutate(rng, g0, 0.01)]
    elif kind == "reads":
        g0 = util.random_genome(rng, 5000)
        seqs = util.reads_from(rng, g0, 4000, 60, err=0.01) + [g0[100:160].copy() for _ in range(30)]   # exact duplicates: sentinel order decides
    elif kind == "copies":
        g0 = util.random_genome(rng, 30000)
        seqs = [g0.copy() for _ in range(5)] + [g0[:777].copy(), g0[29000:].copy()]                       # identical strings: every doubling round is needed
    elif kind == "tiny":
        seqs = [np.array([1, 3, 3], dtype=np.uint8), np.array([1, 3, 2], dtype=np.uint8)]
    elif kind == "runs":
        seqs = [np.full(70000, 1, dtype=np.uint8), np.tile(np.array([1, 2], dtype=np.uint8), 20000), np.full(100, 5, dtype=np.uint8), np.full(70001, 1, dtype=np.uint8)]
    else:
        g0 = util.random_genome(rng, 40000)
        seqs = [util.mutate(rng, g0, 0.002) for _ in range(8)]
    for both in (True, False):
        text = util.make_text(seqs, True, both)
        want = host.build_bwt(text.copy())
        model = sort_model.sort(text)
        h = Rb3Gpu(verbose=1)
        try:
            rounds0 = h.stats()["n_sort_rounds"]
            for step in (0, 100):
                p, ck = h.bwt_from_text(text, step)
                got = h.dev_download(p, text.size)
                h.dev_free(p)
                assert np.array_equal(got, want), (kind, both, step)
                if step:
                    _, w = host.build_bwt_walkers(text.copy(), step)
                    inner = w[w[:, 1] == -1]                # walkers strictly inside strings: their rows are ISA samples
                    assert set(inner[:, 0].tolist()) <= set(ck.tolist())
                    assert len(set(ck.tolist())) == ck.size and ck.min() >= 0 and ck.max() < text.size
                    assert np.array_equal(ck, model.ckrow(step)), (kind, both)
            assert h.stats()["n_sort_rounds"] - rounds0 == 2 * model.rounds, (kind, both)
        finally:
            h.close()


def test_sorter_object_matches_handle_sorter():
    """rb3gpu_sorter_* (a sorter with its own stream and output buffers, used by the CLI's sorter thread): same BWT
    and sampled inverse suffix array as rb3gpu_bwt_from_text; the two output buffers are handed out in turn"""
    import ctypes
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(91)
    h = Rb3Gpu(verbose=1)
    L = h._lib
    s = L.rb3gpu_sorter_create(0)
    assert s
    try:
        held = []
        for rep in range(3):
            g = util.random_genome(rng, int(rng.integers(20000, 90000)))
            text = util.make_text([g, util.mutate(rng, g, 0.01)])
            want = host.build_bwt(text.copy())
            step = 128
            ck = np.empty((text.size + step - 1) // step, dtype=np.int64)
            p = ctypes.c_void_p()
            assert L.rb3gpu_sorter_bwt(s, text.size, text.ctypes.data, ctypes.byref(p), step, ck.ctypes.data) == 0
            got = h.dev_download(p, text.size)
            assert np.array_equal(got, want)
            d2, ck2 = h.bwt_from_text(text, step)
            assert np.array_equal(ck, ck2)
            h.dev_free(d2)
            held.append(p)
            if len(held) == 2:            # both buffers out: give the older one back before the next sort
                assert held[0].value != held[1].value
                assert L.rb3gpu_sorter_release(s, held.pop(0)) == 0
        for p in held:
            assert L.rb3gpu_sorter_release(s, p) == 0
        assert L.rb3gpu_sorter_release(s, held[-1]) != 0   # not out any more
    finally:
        L.rb3gpu_sorter_destroy(s)
        h.close()


def test_whole_index_merge_on_device(oracle):
    """the closing step of the partitioned multi-GPU build (multi.tree_merge) on one GPU: index B is exported as a
    plain BWT into device memory and merged into index A with rb3gpu_merge_plain_dev (the reference's signature, no
    walker list: SA-regular walkers, atomic-min records).  Result = the BWT of all strings in input order."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(97)
    g0 = util.random_genome(rng, 50000)
    gs = [util.mutate(rng, g0, 0.003) for _ in range(8)]
    a, b = Rb3Gpu(verbose=1), Rb3Gpu(verbose=1)
    try:
        for h, part in ((a, gs[:4]), (b, gs[4:])):
            for i, g in enumerate(part):
                bw, w = host.build_bwt_walkers(util.make_text([g]), 256)
                if i == 0: h.from_plain(bw)
                else: h.merge_plain_walkers(bw, w)
        tot = b.get_tot()
        plain_b = b.export_plain()
        d = a.dev_upload(np.zeros(tot + 16, dtype=np.uint8))
        # (two handles on one device: B's export goes through the host here; on two GPUs it is sent over RCCL)
        a._chk(a._lib.rb3gpu_dev_upload(a._h, d, plain_b.ctypes.data, tot), "upload")
        a.merge_plain_dev(d, tot, True)
        a.dev_free(d)
        want = host.build_bwt(util.make_text(gs))
        assert np.array_equal(a.export_plain(), want)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("hook,value", [("pos_limit", 300000), ("win_scratch", 216 * 1200), ("slot_bytes", 128 * 1300)])
def test_size_limits_of_the_single_sync_merge_are_crossed_in_mid_build(oracle, hook, value):
    """the single-synchronisation merge changes regime at sizes no test reaches (merged positions >= 2^38: staged path without
    tentative records; window scratch > 8 GB: group-sequential rebuild; slot upper bound > 16 GB: staged path).  The test build of
    the library shrinks the limits so that a build of a dozen relatives crosses each of them between two merges"""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(163)
    g0 = util.random_genome(rng, 30000)
    gs = [g0] + [util.mutate(rng, g0, 0.003) for _ in range(7)]
    h = Rb3Gpu(verbose=1, hooks=True)
    try:
        h.tune(hook, value)
        want = None
        for i, g in enumerate(gs):
            t = util.make_text([g])
            b = host.build_bwt(t.copy())
            if i == 0:
                h.from_plain(b); want = b
                continue
            if i % 2:
                d_bwt, d_tw = h.sort_text(t)
                h.merge_text_dev(d_bwt, d_tw, t.size, host.walkers_text(t, 200), commit=True)
                h.dev_free(d_bwt); h.dev_free(d_tw)
            else:
                h.merge_plain(b)
            want = oracle.merge(want, b)
            assert np.array_equal(h.export_plain(), want), (hook, i)
        assert h.get_tot() == sum(2 * g.size + 2 for g in gs) > 400000   # (every limit above lies between 300 k and 340 k symbols)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["k2", "k3", "family", "reads"])
def test_pos_equals_the_reference_rb_vectors(oracle, name):
    """pos[] of the HIP rank phase against rb[] >> 6 of the unmodified reference's rb3_mg_rank_plain (committed numbers:
    tests/golden/rb_vectors.npz), through the reference's signature and through the text-order walk"""
    import importlib.util
    from ropebwt3_amd import Rb3Gpu, host
    spec = importlib.util.spec_from_file_location("make_golden_rb", os.path.join(util.ROOT, "tools", "make_golden_rb.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    l1, l2, both = m.cases()[name]
    vec = np.load(os.path.join(util.GOLDEN, "rb_vectors.npz"))
    want, acc_want = vec[name + "_rb"] >> 6, vec[name + "_acc2"]
    t1, t2 = oracle.text(l1, True, both), oracle.text(l2, True, both)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(t1.copy()))
        b2 = host.build_bwt(t2.copy())
        pos, acc2 = h.mg_rank_plain(b2)
        assert np.array_equal(pos, want) and np.array_equal(acc2, acc_want)
        d_bwt, d_tw = h.sort_text(t2)
        n_str = int((t2 == 0).sum())
        for w in ([n_str] if t2.size < 2000 else [n_str, host.walkers_text(t2, 150)]):
            pos2, acc3 = h.mg_rank_text_dev(d_bwt, d_tw, t2.size, w)
            assert np.array_equal(pos2, want) and np.array_equal(acc3, acc_want)
        h.dev_free(d_bwt); h.dev_free(d_tw)
    finally:
        h.close()


def test_forward_strand_upload_equals_full_upload(tmp_path):
    """rb3gpu_sorter_upload_fwd: only the forward strands cross PCIe, the reverse complements (io.c:30-40) are written on the
    device -- the same text in HBM as rb3gpu_sorter_upload, hence the same BWT and inverse suffix array; a text that is not laid
    out as two strands per record is refused"""
    from ropebwt3_amd import Rb3Gpu, Sorter, PinnedArray, Rb3GpuError, host
    rng = np.random.default_rng(151)
    recs = ["".join("ACGTN"[x] for x in rng.choice(5, size=int(n), p=[.25, .25, .25, .24, .01])) for n in (70001, 1, 33333, 2, 12345)]
    fn = tmp_path / "r.fa"
    fn.write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    (n_seq, text), = list(host.read_batches(str(fn), False, 1 << 40))
    pairs = host.strand_pairs(text, n_seq)
    assert pairs is not None and len(pairs) == len(recs) and n_seq == 2 * len(recs)
    h, srt = Rb3Gpu(verbose=1), Sorter(0)
    pin = PinnedArray(text.size)
    pin.array[:] = text
    try:
        out = []
        for src, fwd in ((text, False), (text, True), (pin.array, True), (pin.array, "begin"), (pin.array, "begin+end"), (text, "begin")):
            if fwd == "begin": srt.upload_fwd_begin(src, pairs)          # queued; the sort is ordered behind the copies by the stream
            elif fwd == "begin+end": srt.upload_fwd_begin(src, pairs), srt.upload_end()
            elif fwd: srt.upload_fwd(src, pairs)
            else: srt.upload(src)
            d_bwt, d_tw = srt.sort_uploaded(text.size)
            out.append((h.dev_download(d_bwt, text.size), h.dev_download(d_tw, text.size * 8)))
            srt.release(d_bwt)
        assert np.array_equal(out[0][0], host.build_bwt(text.copy()))
        for o in out[1:]:
            assert np.array_equal(o[0], out[0][0]) and np.array_equal(o[1], out[0][1])
        bad = text.copy()
        bad[pairs[1] - 1] = 1                                # the sentinel of the first reverse strand
        with pytest.raises(Rb3GpuError):
            srt.upload_fwd(bad, pairs)
        assert host.strand_pairs(text[:-3].copy(), n_seq) is None
    finally:
        pin.free(); srt.close(); h.close()


def test_merge_index_between_two_handles(oracle):
    """rb3gpu_merge_index = the tree step of `build --gpus N` (rb3_fmi_merge, fm-index.c:251-277): the index of one handle
    merged into another as one batch, device to device; three slices merged left to right give the BWT of all strings in
    input order, whatever the shape of the tree"""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(131)
    g0 = util.random_genome(rng, 40000)
    gs = [util.mutate(rng, g0, 0.004) for _ in range(9)] + util.reads_from(rng, g0, 30, 80)
    want = host.build_bwt(util.make_text(gs))
    cuts = [0, 3, 7, len(gs)]
    hs = [Rb3Gpu(verbose=1) for _ in range(3)]
    try:
        for h, a, b in zip(hs, cuts[:-1], cuts[1:]):
            for i, g in enumerate(gs[a:b]):
                bw = host.build_bwt(util.make_text([g]))
                if i == 0: h.from_plain(bw)
                else: h.merge_plain(bw)
        hs[0].merge_index(hs[1])
        assert hs[1].get_tot() > 0                       # the source is left as it is
        hs[0].merge_index(hs[2])
        assert np.array_equal(hs[0].export_plain(), want)
        with pytest.raises(Exception):
            hs[0].merge_index(hs[0])
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("entry", ["walkers", "text", "plain"])
def test_full_stretch_table_is_answered_with_fewer_walkers(oracle, entry):
    """a batch whose walkers note more events than the stretch table holds (huge batches into many relatives: the top of the
    multi-GPU tree merge): the merge is done again with every eighth walker before tentative records are given up"""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(137)
    g0 = util.random_genome(rng, 60000)
    rel = [g0] + [util.mutate(rng, g0, 0.004) for _ in range(12)]
    b1 = host.build_bwt(util.make_text(rel))
    t2 = util.make_text([util.mutate(rng, g0, 0.003), util.mutate(rng, g0, 0.003)])
    b2, w = host.build_bwt_walkers(t2.copy(), 150)
    want = oracle.merge(b1, b2)
    h = Rb3Gpu(verbose=1, hooks=True)
    try:
        h.tune("tent_limit", 1200)                        # (blocks of 8 ids per walker: ~800 walkers at spacing 150 do not fit, ~100 at 1200 do)
        h.from_plain(b1)
        if entry == "walkers":
            h.merge_plain_walkers(b2, w)
        elif entry == "text":
            d_bwt, d_tw = h.sort_text(t2)
            h.merge_text_dev(d_bwt, d_tw, t2.size, host.walkers_text(t2, 150), commit=True)
            h.dev_free(d_bwt); h.dev_free(d_tw)
        else:
            h.merge_plain(b2)
        st = h.stats()
        assert np.array_equal(h.export_plain(), want)
        print(entry, "thinned", st["n_thinned"], "fallbacks", st["n_fallbacks"])
        assert st["n_thinned"] >= 1 or st["n_fallbacks"] == 0
    finally:
        h.close()


@pytest.mark.parametrize("env", [{"RB3GPU_GROUP_REBUILD": "1"}, {"RB3GPU_STAGED": "1"}, {"RB3GPU_GROUP_REBUILD": "1", "RB3GPU_STAGED": "1"},
                                 {"RB3GPU_TEXT_MODE": "2"}, {"RB3GPU_WINDOW_REBUILD": "1"}, {"RB3GPU_ABS_LIMIT": "0"}, {"RB3GPU_ABS_LIMIT": "60000"},
                                 {"RB3GPU_B2_SPLIT": "6"}, {"RB3GPU_B2_TW": "0"}, {"RB3GPU_ABS_TABLE": "1"}, {"RB3GPU_B2_SPLIT": "3", "RB3GPU_ABS_TABLE": "1"}])
def test_fallback_code_paths_via_soak(env):
    """the group-sequential rebuild kernels (taken when the window scratch would exceed 8 GB), the staged merge
    (taken for walker-less or oversized merges) and the slot headers of an index of 2^32 symbols or more (counts relative
    to the group; abs_limit moves that border down to nothing or into the middle of the builds) and the splitter spacing that whole-index
    merges of 128 M symbols and more get (b2_split 6), the walk over row words for a batch that came as its BWT only (b2_tw 0: rounds 2-5; the default makes the
    batch's text-order words from its own LF walk) and the layout of 2^32 symbols and more (abs_table: low halves in the headers + the table of bases) forced through the randomised soak"""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "soak.py"), "10", "61000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout.decode()[-2000:]


def test_hundreds_of_relatives(oracle):
    """more matching suffixes (420 near-identical short genomes indexed) than the 255 a tentative walker tracks: the
    walkers stay plain inexact ones until enough relatives have dropped out; same result, no redo"""
    import os
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(101)
    g0 = util.random_genome(rng, 3000)
    rel = [util.mutate(rng, g0, 0.004) for _ in range(420)]
    b1 = host.build_bwt(util.make_text(rel, True, False))
    t2 = util.make_text([util.mutate(rng, g0, 0.004), rel[7].copy(), util.mutate(rng, rel[100], 0.01)], True, False)
    rb, _ = oracle.mg_rank(b1, host.build_bwt(t2.copy()), 8)
    want = rb >> 6
    steps = {}
    for tent, tent_q in (("1", "1"), ("0", "1"), ("1", "2"), ("1", "4")):
        os.environ["RB3GPU_TENT"] = tent
        os.environ["RB3GPU_TENT_Q"] = tent_q
        try:
            h = Rb3Gpu(verbose=1)
            h.from_plain(b1)
            for step in (128, 300):
                b2, w = host.build_bwt_walkers(t2, step)
                got, _ = h.mg_rank_plain_walkers(b2, w)
                assert np.array_equal(got, want), (tent, tent_q, step)
            st = h.stats()
            steps[tent, tent_q] = st["n_lf_steps"] - 2 * want.size
            assert st["n_fallbacks"] == 0
            if tent == "1":
                assert st["tent_mask_bits"] == 256 * int(tent_q), st
            h.close()
        finally:
            os.environ.pop("RB3GPU_TENT", None)
            os.environ.pop("RB3GPU_TENT_Q", None)
    assert steps["1", "1"] <= steps["0", "1"], steps
    # masks of 512 bits track all 420 relatives: the walkers record from their 32nd step on instead of waiting for relatives to drop out
    assert steps["1", "2"] < steps["1", "1"] and steps["1", "4"] <= steps["1", "2"], steps


@pytest.mark.parametrize("seed,kind", [(91, "genome"), (92, "two_strands"), (93, "family"), (94, "copies"), (95, "short")])
def test_merge_text_order_words_vs_oracle(oracle, seed, kind):
    """rb3gpu_merge_text_dev: the batch comes as BWT + text-order words (inverse suffix array) from the GPU sorter and
    the walkers are given by text position; rank phase and merged index bit-exact against the oracle, and the same
    pos[] as the row-word walkers"""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, 60000)
    both = kind != "genome"
    if kind == "family":
        rel = [g0] + [util.mutate(rng, g0, 0.002) for _ in range(11)]
        new = [util.mutate(rng, rel[4], 0.001), rel[7].copy()]
    elif kind == "copies":
        rel = [g0, g0.copy(), util.mutate(rng, g0, 0.01)]
        new = [g0.copy(), g0[:5000].copy(), g0[20000:].copy()]
    elif kind == "short":
        rel = [g0]
        new = [g0[i * 700:i * 700 + 650].copy() for i in range(40)] + [np.array([2], dtype=np.uint8), util.random_genome(rng, 3000)]
    else:
        rel = [g0]
        new = [util.mutate(rng, g0, 0.001)]
    b1 = host.build_bwt(util.make_text(rel, True, both))
    t2 = util.make_text(new, True, both)
    b2 = host.build_bwt(t2.copy())
    rb, _ = oracle.mg_rank(b1, b2, 8)
    want_pos, want = rb >> 6, oracle.merge(b1, b2)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(b1)
        d_bwt, d_tw = h.sort_text(t2)
        assert np.array_equal(h.dev_download(d_bwt, t2.size), b2)
        tw = h.dev_download(d_tw, t2.size * 8).view(np.uint64)
        isa = (tw >> np.uint64(3)).astype(np.int64)
        assert np.array_equal(np.sort(isa), np.arange(t2.size))                     # a permutation: the inverse suffix array
        prev = np.concatenate([[0], t2[:-1]]).astype(np.uint64)
        assert np.array_equal(tw & np.uint64(7), prev) and np.array_equal(b2[isa], prev.astype(np.uint8))
        for step in (100, 384):
            wt = host.walkers_text(t2, step)
            got, acc2 = h.mg_rank_text_dev(d_bwt, d_tw, t2.size, wt)
            assert np.array_equal(got, want_pos), (kind, step)
            assert acc2[6] == t2.size
        assert h.stats()["n_fallbacks"] == 0
        nstr = int((t2 == 0).sum())
        got, _ = h.mg_rank_text_dev(d_bwt, d_tw, t2.size, nstr)                      # one walker per string, made on the device
        assert np.array_equal(got, want_pos), (kind, "per string")
        with pytest.raises(Exception):
            h.mg_rank_text_dev(d_bwt, d_tw, t2.size, nstr + 1)                       # a wrong string count is noticed
        if nstr > 1:
            with pytest.raises(Exception):
                h.mg_rank_text_dev(d_bwt, d_tw, t2.size, nstr - 1)
        if kind == "short":
            h.merge_text_dev(d_bwt, d_tw, t2.size, nstr, commit=True)
        else:
            h.merge_text_dev(d_bwt, d_tw, t2.size, wt, commit=True)
        assert np.array_equal(h.export_plain(), want)
        h2 = Rb3Gpu(verbose=1)                                                       # row words, one walker per string made on the device
        h2.from_plain(b1)
        d2 = h2.dev_upload(b2)
        with pytest.raises(Exception):
            h2.merge_plain_dev_walkers(d2, b2.size, nstr + 3, commit=True)
        h2.merge_plain_dev_walkers(d2, b2.size, nstr, commit=True)
        assert np.array_equal(h2.export_plain(), want)
        h2.dev_free(d2)
        h2.close()
        h.dev_free(d_bwt); h.dev_free(d_tw)
    finally:
        h.close()


@pytest.mark.parametrize("env", [{"force_fallback": 1}, {"tent_limit": 40}, {"staged": 1}, {"tent": 0},
                                 {"text_mode": 2}, {"text_mode": 2, "tent": 0}, {"text_mode": 1}, {"window_rebuild": 1}])
def test_merge_text_order_fallback_paths(oracle, env):
    """the redo path, a stretch table that runs out, the staged path and the walk without tentative records, all
    entered from rb3gpu_merge_text_dev (the walkers are converted to rows on the device where row words are walked)"""
    import os
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(97)
    g0 = util.random_genome(rng, 50000)
    rel = [g0] + [util.mutate(rng, g0, 0.003) for _ in range(7)]
    b1 = host.build_bwt(util.make_text(rel))
    t2 = util.make_text([util.mutate(rng, g0, 0.002), rel[3].copy()])
    want = oracle.merge(b1, host.build_bwt(t2.copy()))
    try:
        h = Rb3Gpu(verbose=1, hooks=True)
        for k, v in env.items():
            h.tune(k, v)
        h.from_plain(b1)
        d_bwt, d_tw = h.sort_text(t2)
        h.merge_text_dev(d_bwt, d_tw, t2.size, host.walkers_text(t2, 200), commit=True)
        st = h.stats()
        assert np.array_equal(h.export_plain(), want)
        if "force_fallback" in env:
            assert st["n_fallbacks"] == 1
        h.close()
    finally:
        pass


def test_config2_full_size_properties_and_oracle(oracle):
    """BASELINE configs[1] at full size (the bench workload: a 4.4 Mbp genome, both strands, merged into the index of a
    0.1 %-divergent one; 8,800,002 symbols each).  Size-independent properties of the interleave -- pos[] strictly
    increasing, ka = pos - row non-decreasing and <= n1, the merged BWT restricted to pos[] is B2 and the rest is B1
    in order, symbol counts add up -- for the text-order walk, and the same pos[] from the row-word walkers and the
    reference-signature entry point; then the merged BWT byte for byte against the oracle."""
    from ropebwt3_amd import Rb3Gpu, host
    g0 = util.random_genome(np.random.default_rng(1), 4400000)
    g1 = util.mutate(np.random.default_rng(2), g0, 0.001)
    b1 = host.build_bwt(util.make_text([g0]))
    t2 = util.make_text([g1])
    b2, w = host.build_bwt_walkers(t2.copy(), 384)
    n1, n2 = b1.size, b2.size
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(b1)
        d_bwt, d_tw = h.sort_text(t2)
        assert np.array_equal(h.dev_download(d_bwt, n2), b2)
        pos, acc2 = h.mg_rank_text_dev(d_bwt, d_tw, n2, host.walkers_text(t2, 384))
        assert h.stats()["n_fallbacks"] == 0
        assert pos[0] >= 0 and pos[-1] < n1 + n2 and np.all(np.diff(pos) > 0)
        ka = pos - np.arange(n2)
        assert np.all(np.diff(ka) >= 0) and ka[0] >= 0 and ka[-1] <= n1
        assert np.array_equal(np.diff(acc2), np.bincount(b2, minlength=6)[:6])
        p_rows, _ = h.mg_rank_plain_walkers(b2, w)
        assert np.array_equal(p_rows, pos)
        p_abi, _ = h.mg_rank_plain(b2)
        assert np.array_equal(p_abi, pos)
        h.merge_text_dev(d_bwt, d_tw, n2, host.walkers_text(t2, 384), commit=True)
        merged = h.export_plain()
        assert merged.size == n1 + n2
        assert np.array_equal(merged[pos], b2)
        keep = np.ones(merged.size, dtype=bool)
        keep[pos] = False
        assert np.array_equal(merged[keep], b1)
        assert np.array_equal(np.bincount(merged, minlength=6), np.bincount(b1, minlength=6) + np.bincount(b2, minlength=6))
        acc = h.get_acc()
        assert acc[6] == n1 + n2
        h.dev_free(d_bwt); h.dev_free(d_tw)
    finally:
        h.close()
    assert np.array_equal(merged, oracle.merge(b1, b2, 8))


def _golden_fmd_names():
    import json
    man = json.load(open(os.path.join(util.GOLDEN, "MANIFEST.json")))
    return sorted(k for k, v in man.items() if isinstance(v, dict) and "fmd" in v and "plain_md5" in v)


@pytest.mark.parametrize("name", _golden_fmd_names())
def test_fmd_decoded_on_the_device(name):
    """rb3gpu_from_fmd_words: the reference's own .fmd files (tests/golden) decoded on the device, one thread per 64-byte
    block: the plain BWT that comes out has the md5 the reference's decoder gives (MANIFEST plain_md5), and the
    symbol counts of the file header"""
    import json, hashlib
    from ropebwt3_amd import Rb3Gpu
    ent = json.load(open(os.path.join(util.GOLDEN, "MANIFEST.json")))[name]
    h = Rb3Gpu(verbose=1)
    try:
        h.from_fmd_file(os.path.join(util.GOLDEN, ent["fmd"]))
        got = h.export_plain()
        assert got.size == ent["n_symbols"]
        text = np.frombuffer(b"$ACGTN", dtype=np.uint8)[got].tobytes() + b"\n"
        assert hashlib.md5(text).hexdigest() == ent["plain_md5"]
    finally:
        h.close()


@pytest.mark.parametrize("name", ["genomes12", "reads_fwd", "copies3000", "longruns", "edge_chars"])
@pytest.mark.parametrize("chunk", [1, 3])
def test_fmd_loaded_in_chunks_without_expanding_it(name, chunk):
    """a large .fmd is decoded and built chunk by chunk (never one byte per symbol for the whole index; rb3_enc_fmd2fmr streams the
    runs too, fm-index.c:56-85): with chunks of 1 or 3 groups the golden files take that path -- the same symbols, the same slot
    partition (index bytes), the same ranks and the same header kind as the one-pass load"""
    import json
    from ropebwt3_amd import Rb3Gpu
    ent = json.load(open(os.path.join(util.GOLDEN, "MANIFEST.json")))[name]
    fn = os.path.join(util.GOLDEN, ent["fmd"])
    a, b = Rb3Gpu(verbose=1), Rb3Gpu(verbose=1)
    try:
        a.tune("load_chunk", 1 << 20)
        a.from_fmd_file(fn)
        b.tune("load_chunk", chunk)
        b.from_fmd_file(fn)
        want = a.export_plain()
        assert want.size == ent["n_symbols"] and np.array_equal(b.export_plain(), want)
        assert a.stats()["bytes_index"] == b.stats()["bytes_index"] and np.array_equal(a.get_acc(), b.get_acc())
        k = np.unique(np.concatenate([np.arange(0, want.size + 1, 997), [want.size, want.size - 1, 8192, 8191, 16384]]).clip(0, want.size))
        assert np.array_equal(a.rank1a(k), b.rank1a(k))
        # and the index merges like any other (text-order walk against the chunk-built block array)
        rng = np.random.default_rng(3)
        t = util.make_text([util.random_genome(rng, 3000)])
        for h in (a, b):
            d_bwt, d_tw = h.sort_text(t)
            h.merge_text_dev(d_bwt, d_tw, t.size, 2, commit=True)
            h.dev_free(d_bwt); h.dev_free(d_tw)
        assert np.array_equal(a.export_plain(), b.export_plain())
    finally:
        a.close(); b.close()


def test_fmd_decode_long_runs_and_garbage():
    """runs longer than 64 k symbols are written by whole workgroups; a stream that is not FMD is refused"""
    from ropebwt3_amd import Rb3Gpu, host
    import subprocess, tempfile
    rng = np.random.default_rng(5)
    seqs = [np.full(300000, 1, dtype=np.uint8), np.full(70000, 3, dtype=np.uint8), util.random_genome(rng, 5000), np.full(200001, 1, dtype=np.uint8)]
    bwt = host.build_bwt(util.make_text(seqs, True, False))
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(bwt)
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "x.txt")
            with open(fa, "wb") as f:
                for s in seqs:
                    f.write(np.frombuffer(b"$ACGTN", dtype=np.uint8)[s].tobytes() + b"\n")
            fmd = os.path.join(d, "x.fmd")
            cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ropebwt3_amd", "ropebwt3-amd")
            subprocess.check_call([cli, "build", "-LR", "-d", "-o", fmd, fa], stderr=subprocess.DEVNULL)
            h2 = Rb3Gpu(verbose=1)
            h2.from_fmd_file(fmd)
            assert np.array_equal(h2.export_plain(), bwt)
            junk = np.frombuffer(rng.integers(0, 256, size=4096, dtype=np.uint8).tobytes(), dtype=np.uint64).copy()
            junk[0] |= np.uint64(3) << np.uint64(62)   # block type 3 does not exist
            with pytest.raises(Exception):
                h2._chk(h2._lib.rb3gpu_from_fmd_words(h2._h, junk.size, junk.ctypes.data, None), "rb3gpu_from_fmd_words")
            h2.close()
    finally:
        h.close()


@pytest.mark.parametrize("seed,nrel,L,per,force", [(201, 24, 30000, 1, 1), (202, 40, 20000, 2, 1), (203, 12, 60000, 1, 1), (204, 64, 9000, 4, 1),
                                                   (205, 130, 5000, 1, 0), (206, 60, 12000, 1, 0)])
def test_run_space_rebuild_vs_oracle_and_window_rebuild(oracle, seed, nrel, L, per, force):
    """the rebuild in run space (k_reb_group: one wave per 8192-symbol group works on the old runs and the batch rows,
    no symbol is regenerated) against the oracle's merge (fm-index.c:237-249) round by round on a family of relatives --
    the index turns from bit planes to run slots as relatives accumulate, so both tiers, the hand-over to the window
    kernels and k_place are exercised -- and against the per-window rebuild (rb3gpu_tune window_rebuild=1): same slots
    statistics, same BWT."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, L)
    rel = []
    for i in range(nrel):
        g = util.mutate(rng, g0, float(rng.choice([0.0005, 0.001, 0.003])))
        if i % 5 == 4:   # an indel, and a long homopolymer now and then
            p = int(rng.integers(0, len(g) - 10))
            g = np.concatenate([g[:p], util.random_genome(rng, int(rng.integers(1, 400))), g[p:]])
        if i % 7 == 6:
            p = int(rng.integers(0, len(g) - 10))
            g = np.concatenate([g[:p], np.full(int(rng.integers(100, 20000)), int(rng.integers(1, 5)), dtype=np.uint8), g[p:]])
        if i % 9 == 8:
            g = rel[int(rng.integers(0, len(rel)))].copy()   # an exact duplicate
        rel.append(g)
    ha, hb = Rb3Gpu(verbose=1), Rb3Gpu(verbose=1)
    hb.tune("window_rebuild", 1)
    ha.tune("reb_force", force)   # 1: also where the host would not start it (many rows per group, index mostly bit planes): the hand-over paths
    want = None
    try:
        for i in range(0, nrel, per):
            t = util.make_text(rel[i:i + per])
            b = host.build_bwt(t.copy())
            if want is None:
                ha.from_plain(b), hb.from_plain(b)
                want = b
                continue
            want = oracle.merge(want, b)
            for h in (ha, hb):
                d, dtw = h.sort_text(t)
                h.merge_text_dev(d, dtw, t.size, host.walkers_text(t, 256), commit=True)
                h.dev_free(d), h.dev_free(dtw)
            ga = ha.export_plain()
            assert np.array_equal(ga, want), ("run-space rebuild", i)
            if (i // per) % 4 == 0:
                assert np.array_equal(hb.export_plain(), want), ("window rebuild", i)
                assert ha.stats()["bytes_index"] == hb.stats()["bytes_index"], i   # the same slot partition
        st = ha.stats()
        assert st["n_fallbacks"] == 0
        print("groups through the run-space rebuild: %d, handed on to the window kernels: %d" % (st["n_reb_groups"], st["n_reb_groups_window"]))
        assert st["n_reb_groups"] > 0
        if nrel >= 24:
            assert st["n_reb_groups_window"] < st["n_reb_groups"], st   # the run-space kernel really did groups
        if not force:
            assert st["n_reb_groups_window"] * 4 < st["n_reb_groups"], st   # where the host starts it by itself, most groups qualify
        assert hb.stats()["n_reb_groups"] == 0
        # rank on the rebuilt index (headers, directory): every 997th offset and the ends
        ks = np.concatenate([np.arange(0, want.size, 997), [want.size - 1, want.size]])
        ok = ha.rank1a(ks)
        cum = np.zeros((want.size + 1, 6), dtype=np.int64)
        for c in range(6):
            cum[1:, c] = np.cumsum(want == c)
        assert np.array_equal(ok, cum[ks])
    finally:
        ha.close(), hb.close()


@pytest.mark.parametrize("key,val", [("reb_lcap", 1), ("reb_slot_cap", 8)])
def test_rebuild_buffers_sized_by_estimates_overflow(oracle, key, val):
    """the single-sync merge sizes two buffers by estimates, because device memory is expensive to obtain and a growing index
    obtains it again and again: the scratch of the window kernels behind the run-space rebuild (room for a fraction of the
    groups) and the slot array (old slots + a margin).  When the device finds that either does not take the result, no
    kernel emits anything and the host does the rebuild again with full sizes.  The test-hook library shrinks the two
    capacities so that every merge goes that way; the result must still equal the oracle's merge (fm-index.c:237-249)."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(77)
    g0 = util.random_genome(rng, 30000)
    rel = [util.mutate(rng, g0, float(rng.choice([0.002, 0.01]))) for _ in range(16)]
    h = Rb3Gpu(verbose=1, hooks=True)
    h.tune("reb_force", 1)
    h.tune(key, val)
    try:
        want = None
        for g in rel:
            t = util.make_text([g])
            b = host.build_bwt(t.copy())
            if want is None:
                h.from_plain(b)
                want = b
                continue
            want = oracle.merge(want, b)
            d, dtw = h.sort_text(t)
            h.merge_text_dev(d, dtw, t.size, host.walkers_text(t, 256), commit=True)
            h.dev_free(d), h.dev_free(dtw)
            assert np.array_equal(h.export_plain(), want)
        st = h.stats()
        assert st["n_reb_again"] >= 3, st
        assert st["n_fallbacks"] == 0
    finally:
        h.close()


@pytest.mark.parametrize("world,kind", [(2, "reads"), (3, "reads"), (2, "family"), (4, "dups")])
def test_interval_sharded_merge_real_engine(oracle, world, kind):
    """north_star multi-GPU split (ropebwt3_amd.multi.merge_interval) driven through the REAL engine: `world` ranks as
    threads of this process, each with its own handle (own HIP stream) holding one interval of the accumulated BWT; the
    collectives are barriers + device-to-device copies (multi.ThreadComm).  Batches of short strings are merged in lock
    step (rb3gpu_sh_step per symbol, states routed to the owner of their insertion point, rb3gpu_sh_finish per interval);
    after every merge the concatenation of the intervals is the oracle's merged BWT, and rank queries on the rebuilt
    intervals agree with it."""
    import threading
    from ropebwt3_amd import Rb3Gpu, host, multi
    rng = np.random.default_rng(300 + world)
    g0 = util.random_genome(rng, 40000)
    if kind == "family":   # a run-coded index: relatives of one genome
        cur = host.build_bwt(util.make_text([util.mutate(rng, g0, 0.002) for _ in range(12)]))
    else:
        cur = host.build_bwt(util.make_text([g0] + util.reads_from(rng, g0, 200, 100)))
    batches = []
    for b in range(3):
        if kind == "dups":
            seqs = [g0[500:650].copy()] * 3 + util.reads_from(rng, g0, 300, 80)
        else:
            seqs = util.reads_from(rng, g0, 2000, int(rng.integers(40, 151)), err=0.01)
        batches.append(util.make_text(seqs, rev=(b != 1)))
    want = [cur]
    for t2 in batches:
        want.append(oracle.merge(want[-1], host.build_bwt(t2.copy())))
    shared = multi.ThreadComm.Shared(world)
    bounds0 = multi.interval_bounds(cur.size, world)
    errs, rounds = [], [None] * world

    def run(rank):
        try:
            h = Rb3Gpu(verbose=1)
            comm = multi.ThreadComm(shared, rank, h)
            bounds = bounds0
            h.from_plain(cur[bounds[rank]:bounds[rank + 1]])
            for b, t2 in enumerate(batches):
                d_bwt, d_tw = h.sort_text(t2)
                st = {}
                bounds = multi.merge_interval(h, comm, bounds, d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0), commit=True, stats=st)
                h.dev_free(d_bwt), h.dev_free(d_tw)
                w = want[b + 1]
                assert bounds[-1] == w.size
                mine = w[bounds[rank]:bounds[rank + 1]]
                assert h.get_tot() == mine.size
                assert np.array_equal(h.export_plain(), mine), (rank, b)
                ks = np.unique(np.concatenate([rng.integers(0, mine.size + 1, size=50), [0, mine.size]]))
                cum = np.stack([np.concatenate([[0], np.cumsum(mine == c)]) for c in range(6)], axis=1)
                assert np.array_equal(h.rank1a(ks), cum[ks])
                rounds[rank] = st["rounds"]
            h.close()
        except BaseException as e:   # (a failed rank must not leave the others waiting at the barrier for ever)
            errs.append((rank, repr(e)))
            shared.barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not errs, errs
    assert all(r == rounds[0] for r in rounds) and rounds[0] >= 40


def _sharded_case(oracle, rng, kind):
    """(index BWT, batches as texts, merged BWT after every batch) of the interval-sharded tests"""
    from ropebwt3_amd import host
    g0 = util.random_genome(rng, 40000)
    if kind == "family":   # a run-coded index: relatives of one genome
        cur = host.build_bwt(util.make_text([util.mutate(rng, g0, 0.002) for _ in range(12)]))
    else:
        cur = host.build_bwt(util.make_text([g0] + util.reads_from(rng, g0, 200, 100)))
    batches = []
    for b in range(3):
        if kind == "dups":
            seqs = [g0[500:650].copy()] * 3 + util.reads_from(rng, g0, 300, 80)
        elif kind == "ragged":   # strings of very different lengths, one of them a single symbol
            seqs = [util.mutate(rng, g0, 0.01)[:3000], g0[5:6].copy(), util.mutate(rng, g0, 0.02)[1000:1100]] + util.reads_from(rng, g0, 50, 60)
        else:
            seqs = util.reads_from(rng, g0, 2000, int(rng.integers(40, 151)), err=0.01)
        batches.append(util.make_text(seqs, rev=(b != 1)))
    want = [cur]
    for t2 in batches:
        want.append(oracle.merge(want[-1], host.build_bwt(t2.copy())))
    return cur, batches, want


def _check_interval(h, rng, w, bounds, rank):
    assert bounds[-1] == w.size
    mine = w[bounds[rank]:bounds[rank + 1]]
    assert h.get_tot() == mine.size
    assert np.array_equal(h.export_plain(), mine)
    ks = np.unique(np.concatenate([rng.integers(0, mine.size + 1, size=50), [0, mine.size]]))
    cum = np.stack([np.concatenate([[0], np.cumsum(mine == c)]) for c in range(6)], axis=1)
    assert np.array_equal(h.rank1a(ks), cum[ks])


@pytest.mark.parametrize("world,kind", [(1, "reads"), (2, "reads"), (3, "reads"), (2, "family"), (4, "dups"), (3, "ragged")])
def test_interval_sharded_merge_driven_from_the_library(oracle, world, kind):
    """rb3gpu_sh_merge: the lock-step loop of the interval-sharded merge INSIDE the library (one k_sh_round per symbol, split
    sizes read back, all-gather + all-to-all through the library's own thread-group communicator: barriers + device-to-device
    copies), `world` ranks as threads with a handle each.  After every merge the concatenation of the intervals is the oracle's
    merged BWT, rank queries on the rebuilt intervals agree with it, and a merge with commit=False leaves everything as it was."""
    import threading
    from ropebwt3_amd import Rb3Gpu, CommGroup, multi
    rng = np.random.default_rng(500 + world)
    cur, batches, want = _sharded_case(oracle, rng, kind)
    bounds0 = multi.interval_bounds(cur.size, world)
    grp = CommGroup(world)
    errs, rounds = [], [None] * world

    def run(rank):
        try:
            r = np.random.default_rng(900 + rank)
            h = Rb3Gpu(verbose=1)
            comm = grp.comm(rank, h)
            bounds = bounds0
            h.from_plain(cur[bounds[rank]:bounds[rank + 1]])
            for b, t2 in enumerate(batches):
                d_bwt, d_tw = h.sort_text(t2)
                sent = np.flatnonzero(t2 == 0)
                if b == 1:   # a dry run first: nothing may change
                    nb, _ = h.sh_merge(comm, bounds, d_bwt, d_tw, t2.size, sent, commit=False)
                    assert np.array_equal(nb, bounds)
                    _check_interval(h, r, want[b], bounds, rank)
                bounds, nr = h.sh_merge(comm, bounds, d_bwt, d_tw, t2.size, sent, commit=True)
                h.dev_free(d_bwt), h.dev_free(d_tw)
                _check_interval(h, r, want[b + 1], bounds, rank)
                rounds[rank] = nr
            h.close()
        except BaseException as e:   # (a failed rank must not leave the others waiting at the barrier for ever)
            errs.append((rank, repr(e)))
            grp.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    grp.close()
    assert not errs, errs
    longest = int(np.max(np.diff(np.concatenate([[-1], np.flatnonzero(batches[-1] == 0)]))))
    assert all(r == longest for r in rounds), (rounds, longest)   # one round per symbol of the longest string, its sentinel included


@pytest.mark.parametrize("states,block", [(0, 0), (8, 256), (4, 0), (2, 0)])
def test_interval_sharded_merge_many_chains(oracle, states, block):
    """600 k chains of ragged lengths (4..40 symbols) in one batch, two intervals: the round kernel with the launch shape the library picks
    (k_sh_round<8, 1024> from 2^15 live chains on, one state per octet below: the launch follows the number of live chains as they end) and
    with the other instantiations asked for through the tune keys (sh_states, sh_block)"""
    import threading
    from ropebwt3_amd import Rb3Gpu, CommGroup, host, multi
    world = 2
    rng = np.random.default_rng(2024)
    g0 = util.random_genome(rng, 200000)
    cur = host.build_bwt(util.make_text([g0]))
    n = 300000
    st, ln = rng.integers(0, len(g0) - 40, size=n), rng.integers(4, 41, size=n)
    t2 = util.make_text([g0[a:a + l] for a, l in zip(st, ln)])
    want = oracle.merge(cur, host.build_bwt(t2.copy()))
    bounds0 = multi.interval_bounds(cur.size, world)
    grp = CommGroup(world)
    errs = []

    def run(rank):
        try:
            h = Rb3Gpu(verbose=1)
            if states:
                h.tune("sh_states", states)
            if block:
                h.tune("sh_block", block)
            comm = grp.comm(rank, h)
            h.from_plain(cur[bounds0[rank]:bounds0[rank + 1]])
            d_bwt, d_tw = h.sort_text(t2)
            bounds, nr = h.sh_merge(comm, bounds0, d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
            assert nr == 41
            _check_interval(h, np.random.default_rng(rank), want, bounds, rank)
            h.close()
        except BaseException as e:
            errs.append((rank, repr(e)))
            grp.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    grp.close()
    assert not errs, errs


@pytest.mark.parametrize("world,skew", [(2, False), (4, False), (4, True)])
def test_interval_sharded_merge_peer_rounds(oracle, world, skew):
    """PEER ROUNDS (rb3gpu_comm_t.stream_barrier; the thread-group communicator offers it): the lock-step rounds as one kernel per rank that writes the
    next states straight into the owners' receive buffers -- every round counted in n_peer_rounds, the merged intervals the oracle's, and the same
    intervals from the same merge with the rounds driven by the host (tune sh_host_rounds: every rank must say so, they agree on the path).
    skew: three intervals of a few symbols and one with the rest, so that more rows land in it than the peer rounds made room for (three times a
    rank's share): they give up on the device, say so, and the merge is done again the old way -- same result, no peer round counted."""
    import threading
    from ropebwt3_amd import Rb3Gpu, CommGroup, host, multi
    rng = np.random.default_rng(77 + world)
    g0 = util.random_genome(rng, 60000)
    cur = host.build_bwt(util.make_text([g0]))
    n = 14000 if skew else 3000
    st, ln = rng.integers(0, len(g0) - 60, size=n), rng.integers(20, 61, size=n)
    t2 = util.make_text([g0[a:a + l] for a, l in zip(st, ln)])
    want = oracle.merge(cur, host.build_bwt(t2.copy()))
    if skew:
        assert t2.size > 3 * (t2.size // world) + (1 << 16) + 4000
        bounds0 = np.array([0, 700, 1500, 2100, cur.size], dtype=np.int64)
    else:
        bounds0 = multi.interval_bounds(cur.size, world)
    sent = np.flatnonzero(t2 == 0)
    longest = int(np.max(np.diff(np.concatenate([[-1], sent]))))
    res = {}
    for host_rounds in (0, 1):
        grp = CommGroup(world)
        errs, out = [], [None] * world

        def run(rank):
            try:
                h = Rb3Gpu(verbose=1)
                if host_rounds:
                    h.tune("sh_host_rounds", 1)
                comm = grp.comm(rank, h)
                assert comm.struct.stream_barrier
                h.from_plain(cur[bounds0[rank]:bounds0[rank + 1]])
                d_bwt, d_tw = h.sort_text(t2)
                bounds, nr = h.sh_merge(comm, bounds0, d_bwt, d_tw, t2.size, sent)
                assert nr == longest
                _check_interval(h, np.random.default_rng(rank), want, bounds, rank)
                out[rank] = (h.stats()["n_peer_rounds"], bounds.copy(), h.export_plain())
                h.dev_free(d_bwt), h.dev_free(d_tw)
                h.close()
            except BaseException as e:
                errs.append((rank, repr(e)))
                grp.abort()

        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=600)
        grp.close()
        assert not errs, errs
        res[host_rounds] = out
    for rank in range(world):
        assert res[0][rank][0] == (0 if skew else longest) and res[1][rank][0] == 0, [x[0] for x in res[0]]
        assert np.array_equal(res[0][rank][1], res[1][rank][1]) and np.array_equal(res[0][rank][2], res[1][rank][2])
    assert np.array_equal(np.concatenate([x[2] for x in res[0]]), want)


@pytest.mark.parametrize("kind", ["random", "copies", "mixed"])
def test_fmd_packed_a_piece_at_a_time(kind):
    """rb3gpu_export_fmd_words packs the runs a PIECE at a time (rb3fmd_enc_*, round 6: device memory per run of a piece, not of the index): with pieces of
    32 k runs (tune fmd_piece; 64 M by default) -- dozens of pieces, each handing its last complete block, the block that has begun and the run whose end is
    not known yet to the next -- the word stream is the one a single piece gives, which every .fmd test holds against the reference's bytes.
    random: short runs, 16-bit block headers; copies: runs of thousands, mostly 32-bit headers; mixed: a repetitive part in front of a random one."""
    from ropebwt3_amd import Rb3Gpu
    rng = np.random.default_rng({"random": 1, "copies": 2, "mixed": 3}[kind])
    if kind == "random":
        t = util.make_text([util.random_genome(rng, 1500000)], rev=False)
    elif kind == "copies":
        g = util.random_genome(rng, 50000)
        t = util.make_text([util.mutate(rng, g, 0.0001) for _ in range(3000)], rev=False)
    else:
        g = util.random_genome(rng, 8000)
        t = util.make_text([util.mutate(rng, g, 0.0004) for _ in range(1200)] + [util.random_genome(rng, 400000)], rev=False)
    h = Rb3Gpu(verbose=1)
    try:
        d, dtw = h.sort_text(t)
        h.from_plain_dev(d, t.size)
        h.dev_free(d), h.dev_free(dtw)
        one = h.export_fmd_words()
        runs = int(np.count_nonzero(np.diff(h.export_plain().astype(np.int16))) + 1)
        assert runs > 2 * 32768, runs
        for piece in (32768, 50000):
            h.tune("fmd_piece", piece)
            many = h.export_fmd_words()
            assert many.size == one.size and np.array_equal(many, one), (kind, piece, runs, many.size, one.size)
        types = {int(one[8 * b] >> 62) for b in range(1, one.size // 8, 97)}
        assert (types == {0}) if kind == "random" else (1 in types) if kind == "copies" else True, types   # (16-bit headers only / blocks of 16 k symbols and more among them)
    finally:
        h.close()


def test_buffer_bytes_account_for_the_handle(oracle):
    """rb3gpu_buffer_bytes: the buffers a handle reports add up to no more than its peak, the current slot array holds the index, and the
    stretch table is there at its fixed size once a merge with tentative records has run"""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(5)
    g = util.random_genome(rng, 300000)
    t1, t2 = util.make_text([g]), util.make_text([util.mutate(rng, g, 0.002)])
    h = Rb3Gpu(verbose=1)
    try:
        d, dtw = h.sort_text(t1)
        h.from_plain_dev(d, t1.size)
        h.dev_free(d), h.dev_free(dtw)
        d, dtw = h.sort_text(t2)
        h.merge_text_dev(d, dtw, t2.size, host.walkers_text(t2, 192), commit=True)
        h.dev_free(d), h.dev_free(dtw)
        b, st = h.buffers(), h.stats()
        assert b and all(v > 0 for v in b.values())
        assert sum(b.values()) <= st["bytes_peak"]
        assert b["index slots (current)"] + b["index directory (current)"] >= st["bytes_index"]
        assert 16777216 * 68 <= b["dl (stretch table)"] <= 16777216 * 68 + 4096
    finally:
        h.close()


def test_shard_object_split_merge_gather(oracle):
    """rb3gpu_shard_*: what the CLI's --interval mode calls -- split the index of a handle into intervals (device-to-device copies
    of its plain symbols), merge batches with a thread per interval inside the library, gather: the handle then holds the oracle's
    merged BWT and exports it like any other"""
    from ropebwt3_amd import Rb3Gpu, Shard
    rng = np.random.default_rng(4)
    cur, batches, want = _sharded_case(oracle, rng, "reads")
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(cur)
        sh = Shard(h, [0, 0, 0])
        b = sh.bounds()
        assert b[0] == 0 and b[-1] == cur.size and np.all(np.diff(b) > 0)
        for t2 in batches:
            d_bwt, d_tw = h.sort_text(t2)
            sh.merge(d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
            h.dev_free(d_bwt), h.dev_free(d_tw)
        assert sh.bounds()[-1] == want[-1].size and h.get_tot() == sh.bounds()[1]   # the handle holds its interval only
        sh.gather()
        assert h.get_tot() == want[-1].size
        assert np.array_equal(h.export_plain(), want[-1])
    finally:
        h.close()


def test_shard_object_exports_without_a_gather(oracle):
    """the writers' view of the sharded index: runs taken from the intervals in rank order and joined at the seams (rb3gpu_shard_export_runs /
    _run_words), cumulative counts summed over the intervals -- the oracle's merged BWT, with no interval ever copied to another device.
    A run-coded index (relatives) cut by BYTES of the block array, not by symbols; and the batch sharded inside rb3gpu_shard_merge."""
    from ropebwt3_amd import Rb3Gpu, Shard
    for kind, nd in (("family", 3), ("reads", 4), ("dups", 2)):
        rng = np.random.default_rng(40 + nd)
        cur, batches, want = _sharded_case(oracle, rng, kind)
        h = Rb3Gpu(verbose=1)
        try:
            h.from_plain(cur)
            sh = Shard(h, [0] * nd)
            for t2 in batches:
                d_bwt, d_tw = h.sort_text(t2)
                sh.merge(d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
                h.dev_free(d_bwt), h.dev_free(d_tw)
            w = want[-1]
            assert np.array_equal(sh.export_plain(), w), kind
            st, sy, end = sh.export_run_words()
            assert end == w.size
            chg = np.flatnonzero(np.concatenate([[True], w[1:] != w[:-1]]))
            assert np.array_equal(st, chg) and np.array_equal(sy, w[chg]), kind
            acc = sh.get_acc()
            assert np.array_equal(np.diff(acc), np.bincount(w, minlength=6)[:6])
            sh.destroy()
            assert h.get_tot() < w.size     # the handle still holds its own interval only
        finally:
            h.close()


def test_shard_rebalance_moves_the_bounds_to_equal_bytes(oracle, monkeypatch):
    """rb3gpu_shard_rebalance ("rebalance by neighbour shifts when the largest interval exceeds the mean by 25 %"): an index whose
    second half is incompressible and whose first half is one run, cut into four intervals of equal SYMBOL counts by hand (two nearly empty
    of bytes, two heavy), is rebalanced to intervals of about equal bytes; the index is the same symbol for symbol, merges go on afterwards,
    and a balanced index is left alone."""
    from ropebwt3_amd import Rb3Gpu, Shard, host
    monkeypatch.setenv("RB3GPU_SHARD_REBALANCE_PCT", "-1")      # not by itself inside merge(): this test calls it
    rng = np.random.default_rng(9)
    g0 = util.random_genome(rng, 60000)
    cur = host.build_bwt(util.make_text([g0] + [util.mutate(rng, g0, 0.001) for _ in range(30)], rev=False))   # runs of ~30: compressible ...
    t2s = [util.make_text(util.reads_from(rng, util.random_genome(rng, 40000), 3000, 120), rev=False) for _ in range(2)]  # ... and batches of unrelated reads: bit planes wherever they land
    want = [cur]
    for t2 in t2s:
        want.append(oracle.merge(want[-1], host.build_bwt(t2.copy())))
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(cur)
        sh = Shard(h, [0, 0, 0, 0])
        assert sh.rebalance(25) == 0                              # cut by bytes a moment ago: nothing to do
        for k, t2 in enumerate(t2s):
            d_bwt, d_tw = h.sort_text(t2)
            sh.merge(d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
            h.dev_free(d_bwt), h.dev_free(d_tw)
        by = np.array([sh.handle_stats(i)["bytes_index"] for i in range(4)], dtype=np.float64)
        did = sh.rebalance(0)                                     # any difference at all
        by2 = np.array([sh.handle_stats(i)["bytes_index"] for i in range(4)], dtype=np.float64)
        assert did == 1 and by2.max() / by2.mean() <= max(1.15, by.max() / by.mean()), (by, by2)
        b = sh.bounds()
        assert b[0] == 0 and b[-1] == want[-1].size and np.all(np.diff(b) > 0)
        assert np.array_equal(sh.export_plain(), want[-1])
        t3 = util.make_text(util.reads_from(rng, g0, 500, 100), rev=True)   # and the rebalanced intervals take another batch
        d_bwt, d_tw = h.sort_text(t3)
        sh.merge(d_bwt, d_tw, t3.size, np.flatnonzero(t3 == 0))
        h.dev_free(d_bwt), h.dev_free(d_tw)
        assert np.array_equal(sh.export_plain(), oracle.merge(want[-1], host.build_bwt(t3.copy())))
        sh.destroy()
    finally:
        h.close()


def test_balanced_bounds_follow_the_bytes_of_the_block_array(oracle):
    """rb3gpu_balanced_bounds: an index whose first half is one long run and whose second half is random symbols is cut where the BYTES
    are (nearly all in the second half), not in the middle"""
    from ropebwt3_amd import Rb3Gpu
    rng = np.random.default_rng(5)
    n = 1 << 21
    b = np.concatenate([np.full(n, 1, dtype=np.uint8), rng.integers(1, 5, size=n).astype(np.uint8), np.zeros(1, dtype=np.uint8)])
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(b)
        bd = h.balanced_bounds(4)
        assert bd[0] == 0 and bd[-1] == b.size and np.all(np.diff(bd) > 0)
        assert bd[1] > n and bd[2] > n      # equal symbol counts would put bd[1] at n / 2 and bd[2] at n
    finally:
        h.close()


@pytest.mark.parametrize("world,kind", [(1, "reads"), (2, "reads"), (3, "family"), (4, "dups"), (3, "ragged")])
def test_interval_sharded_merge_with_a_sharded_batch(oracle, world, kind):
    """rb3gpu_sh_merge_text: every rank holds the symbol-before array (1 byte per batch symbol) and ITS text range of the text-order words
    only; the records are (text position, insertion point) and the rows come back from the owners of the text ranges in one exchange at
    the end.  `world` ranks as threads with a handle each; after every merge the intervals are the oracle's."""
    import threading
    from ropebwt3_amd import Rb3Gpu, CommGroup, multi
    rng = np.random.default_rng(640 + world)
    cur, batches, want = _sharded_case(oracle, rng, kind)
    bounds0 = multi.interval_bounds(cur.size, world)
    grp = CommGroup(world)
    errs = []

    def run(rank):
        try:
            r = np.random.default_rng(900 + rank)
            h = Rb3Gpu(verbose=1)
            comm = grp.comm(rank, h)
            bounds = bounds0
            h.from_plain(cur[bounds[rank]:bounds[rank + 1]])
            for b, t2 in enumerate(batches):
                d_bwt, d_tw = h.sort_text(t2)
                d_tp = h.tprev_from_tw(d_tw, t2.size)
                n2 = t2.size
                t_lo = n2 // world * rank + (n2 % world) * rank // world
                t_hi = n2 if rank + 1 == world else n2 // world * (rank + 1) + (n2 % world) * (rank + 1) // world
                d_slice = h.dev_alloc((t_hi - t_lo) * 8 + 64)      # a copy of the slice: nothing else of the words is reachable through it
                h.dev_copy(d_slice, d_tw.value + t_lo * 8, (t_hi - t_lo) * 8)
                h.dev_memset(d_tw, 0xEE, n2 * 8)                   # ... and the whole array is spoilt
                bounds, _ = h.sh_merge_text(comm, bounds, d_tp, d_slice, n2, np.flatnonzero(t2 == 0), commit=True)
                h.dev_free(d_bwt), h.dev_free(d_tw), h.dev_free(d_tp), h.dev_free(d_slice)
                _check_interval(h, r, want[b + 1], bounds, rank)
            h.close()
        except BaseException as e:
            errs.append((rank, repr(e)))
            grp.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    grp.close()
    assert not errs, errs


def test_shard_object_beside_a_busy_sorter(oracle):
    """the sharded index while ANOTHER thread keeps the device busy with suffix sorting (what the CLI's sorter thread does): the copies
    that cut the index into intervals and put it back together must be complete before the handles read them -- a device-to-device
    hipMemcpy only queues the copy (found at 10 M reads through the CLI: a valid but wrong BWT, one run in three)"""
    import threading
    from ropebwt3_amd import Rb3Gpu, Shard, Sorter
    rng = np.random.default_rng(8)
    g0 = util.random_genome(rng, 2000000)
    t1 = util.make_text(util.reads_from(rng, g0, 60000, 100), rev=False)
    t2 = util.make_text(util.reads_from(rng, g0, 30000, 100), rev=False)
    big = util.make_text([g0])
    stop = []

    def busy():
        s2 = Sorter(0)
        while not stop:
            s2.upload(big)
            d2, _ = s2.sort_uploaded(big.size)
            s2.release(d2)

    th = threading.Thread(target=busy)
    th.start()
    try:
        want = None
        for rep in range(6):
            h = Rb3Gpu(verbose=1)
            d1, d1tw = h.sort_text(t1)
            h.from_plain_dev(d1, t1.size)
            sh = Shard(h, [0, 0, 0, 0])
            d2, d2tw = h.sort_text(t2)
            sh.merge(d2, d2tw, t2.size, np.flatnonzero(t2 == 0))
            sh.gather()
            got = h.export_plain()
            for p in (d1, d1tw, d2, d2tw):
                h.dev_free(p)
            h.close()
            if want is None:
                from ropebwt3_amd import host
                want = oracle.merge(host.build_bwt(t1.copy()), host.build_bwt(t2.copy()))
            assert np.array_equal(got, want), rep
    finally:
        stop.append(1)
        th.join()


def test_interval_sharded_merge_through_callbacks(oracle):
    """the same merge with a communicator made of two Python callables (what a launcher without RCCL -- gloo, MPI -- plugs in):
    two ranks as threads, the all-to-all as device-to-device copies out of the per-destination send regions; and a rank whose
    call fails (wrong bounds) aborts the others instead of leaving them in the barrier"""
    import threading
    from ropebwt3_amd import Rb3Gpu, CallbackComm, Rb3GpuError, multi
    world = 2
    rng = np.random.default_rng(77)
    cur, batches, want = _sharded_case(oracle, rng, "reads")
    bounds0 = multi.interval_bounds(cur.size, world)
    bar = threading.Barrier(world)
    slots, pubs = [None] * world, [None] * world
    errs = []

    def run(rank, sabotage):
        try:
            h = Rb3Gpu(verbose=0)

            def all_gather(vec):
                slots[rank] = vec
                bar.wait()
                out = np.stack(slots)
                bar.wait()
                return out

            def exchange(d_send, stride, send_cnt, d_recv, recv_cnt):
                h.sync()
                pubs[rank] = (d_send, stride, send_cnt)
                bar.wait()
                at = 0
                for src in range(world):
                    p, st, cnt = pubs[src]
                    n = int(cnt[rank])
                    assert n == int(recv_cnt[src])
                    if n:
                        h.dev_copy(d_recv + at * 16, p + rank * st * 16, n * 16)
                    at += n
                h.sync()
                bar.wait()

            comm = CallbackComm(rank, world, all_gather, exchange, abort=bar.abort)
            bounds = bounds0
            h.from_plain(cur[bounds[rank]:bounds[rank + 1]])
            t2 = batches[0]
            d_bwt, d_tw = h.sort_text(t2)
            if sabotage:
                wrong = bounds.copy()
                if rank == 1:
                    wrong[1] += 1   # not the interval the handle holds: EINVAL on this rank, before its first collective
                with pytest.raises(Rb3GpuError):
                    h.sh_merge(comm, wrong, d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
            else:
                bounds, _ = h.sh_merge(comm, bounds, d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
                _check_interval(h, np.random.default_rng(rank), want[1], bounds, rank)
            h.close()
        except BaseException as e:
            errs.append((rank, repr(e)))
            bar.abort()

    for sabotage in (False, True):
        bar.reset()
        th = [threading.Thread(target=run, args=(r, sabotage)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errs, errs


def _gloo_sh_worker(rank, world, port, q, ipc=False):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    from ropebwt3_amd import Rb3Gpu, CallbackComm, multi, host
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        orc = util.Oracle()
        rng = np.random.default_rng(4242)   # the same case on every rank
        cur, batches, want = _sharded_case(orc, rng, "reads")
        bounds = multi.interval_bounds(cur.size, world)
        h = Rb3Gpu(verbose=1)

        def all_gather(vec):
            out = [torch.zeros(len(vec), dtype=torch.int64) for _ in range(world)]
            dist.all_gather(out, torch.from_numpy(np.ascontiguousarray(vec, dtype=np.int64)))
            return torch.stack(out).numpy()

        def exchange(d_send, stride, send_cnt, d_recv, recv_cnt):   # host-staged: gloo moves CPU tensors
            parts = []
            for d in range(world):
                n = int(send_cnt[d])
                parts.append(torch.from_numpy(h.dev_download_i64(d_send + d * stride * 16, n * 2)) if n else torch.zeros(0, dtype=torch.int64))
            recv = [torch.zeros(int(recv_cnt[s]) * 2, dtype=torch.int64) for s in range(world)]
            dist.all_to_all(recv, parts) if dist.get_backend() != "gloo" else _gloo_all_to_all(dist, rank, world, parts, recv)
            got = torch.cat(recv).numpy()
            if got.size:
                h.dev_upload_to(d_recv, got)

        comm = CallbackComm(rank, world, all_gather, exchange)
        if ipc:   # peer rounds between PROCESSES: receive buffers shared through HIP IPC handles, interprocess events, a barrier in shared memory
            from ropebwt3_amd import ipc_peer_enable, ipc_peer_disable
            assert ipc_peer_enable(h, comm) and comm.struct.stream_barrier and comm.struct.peer_import
        h.from_plain(cur[bounds[rank]:bounds[rank + 1]])
        nround = 0
        for b, t2 in enumerate(batches):
            d_bwt, d_tw = h.sort_text(t2)
            bounds, nr = h.sh_merge(comm, bounds, d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
            nround += nr
            h.dev_free(d_bwt), h.dev_free(d_tw)
            _check_interval(h, np.random.default_rng(rank), want[b + 1], bounds, rank)
        if ipc:   # a batch of more chains than any before: every rank replaces its receive buffers -- the other processes give their mappings of them up first
            g0 = util.random_genome(np.random.default_rng(7), 30000)
            t3 = util.make_text(util.reads_from(np.random.default_rng(8), g0, 9000, 60, err=0.01))
            w3 = orc.merge(want[-1], host.build_bwt(t3.copy()))
            d_bwt, d_tw = h.sort_text(t3)
            bounds, nr = h.sh_merge(comm, bounds, d_bwt, d_tw, t3.size, np.flatnonzero(t3 == 0))
            nround += nr
            h.dev_free(d_bwt), h.dev_free(d_tw)
            _check_interval(h, np.random.default_rng(rank), w3, bounds, rank)
        assert h.stats()["n_peer_rounds"] == (nround if ipc else 0), (h.stats()["n_peer_rounds"], nround)
        if ipc:
            ipc_peer_disable(h, comm)
            assert not comm.struct.stream_barrier
        h.close()
        q.put((rank, True, ""))
    except BaseException as e:
        q.put((rank, False, repr(e)))
    finally:
        dist.destroy_process_group()


def _gloo_all_to_all(dist, rank, world, parts, recv):
    """gloo has no all_to_all for CPU tensors of unequal sizes everywhere: pairwise send/recv, lower rank sends first"""
    for peer in range(world):
        if peer == rank:
            recv[rank].copy_(parts[rank])
        elif rank < peer:
            if parts[peer].numel(): dist.send(parts[peer], peer)
            if recv[peer].numel(): dist.recv(recv[peer], peer)
        else:
            if recv[peer].numel(): dist.recv(recv[peer], peer)
            if parts[peer].numel(): dist.send(parts[peer], peer)


def test_interval_sharded_merge_c_path_over_gloo():
    """world 2 as two PROCESSES (sharing this GPU) joined by gloo: rb3gpu_sh_merge runs the loop in the library, the launcher
    only supplies the two collectives"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 2
    procs = [ctx.Process(target=_gloo_sh_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] for r in res), res


@pytest.mark.parametrize("world", [2, 3])
def test_interval_sharded_merge_peer_rounds_between_processes(world):
    """PEER ROUNDS where the ranks are PROCESSES (rb3gpu_ipc_peer_enable over the gloo callbacks; what bench.py --gpus N runs): every rank's receive buffers and
    counter tables mapped into the others through HIP IPC memory handles, interprocess events for the streams, a spin barrier in POSIX shared memory for the
    hosts -- all rounds counted as peer rounds, the intervals the oracle's after every merge"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_sh_worker, args=(r, world, port, q, True)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] for r in res), res


class _GlooGroup:
    """the torch.distributed calls of the gloo callbacks (all_gather, send, recv) on a gloo group of one rank's own: a process can host several ranks"""

    def __init__(self, store, rank, world):
        import torch.distributed as dist
        self.pg = dist.ProcessGroupGloo(dist.PrefixStore("rb3_text", store), rank, world)

    def all_gather(self, out, t):
        self.pg.allgather([out], [t]).wait()

    def send(self, t, dst):
        self.pg.send([t], dst, 0).wait()

    def recv(self, t, src):
        self.pg.recv([t], src, 0).wait()


def _text_ranks_worker(ranks, world, port, q, n_reads):
    """ranks `ranks` of rb3gpu_sh_merge_text between processes, a thread each with an engine handle (and so a stream) and a gloo group of its
    own: the case and the callbacks of tools/probe_gloo_text.worker"""
    import sys
    import threading
    from datetime import timedelta
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    from ropebwt3_amd import Rb3Gpu, CallbackComm, multi, host
    orc = util.Oracle()
    rng = np.random.default_rng(99)   # the same case in every process
    g0 = util.random_genome(rng, 300000)
    cur = host.build_bwt(util.make_text([g0]))
    t2 = util.make_text(util.reads_from(rng, g0, n_reads, 75, err=0.01))
    want = orc.merge(cur, host.build_bwt(t2.copy()))
    stores = {}

    def run(rank):
        try:
            stores[rank] = dist.TCPStore("127.0.0.1", port, world, rank == 0, timedelta(seconds=300), wait_for_workers=False)   # (rank 0's serves)
            g = _GlooGroup(stores[rank], rank, world)
            bounds = multi.interval_bounds(cur.size, world)
            h = Rb3Gpu(verbose=1)

            def all_gather(vec):
                out = [torch.zeros(len(vec), dtype=torch.int64) for _ in range(world)]
                g.all_gather(out, torch.from_numpy(np.ascontiguousarray(vec, dtype=np.int64)))
                return torch.stack(out).numpy()

            def exchange(d_send, stride, send_cnt, d_recv, recv_cnt):   # synchronous copies out of the send regions, right behind the kernel that fills them
                parts = []
                for d in range(world):
                    n = int(send_cnt[d])
                    parts.append(torch.from_numpy(h.dev_download_i64(d_send + d * stride * 16, n * 2)) if n else torch.zeros(0, dtype=torch.int64))
                recv = [torch.zeros(int(recv_cnt[s]) * 2, dtype=torch.int64) for s in range(world)]
                _gloo_all_to_all(g, rank, world, parts, recv)
                got = torch.cat(recv).numpy()
                if got.size:
                    h.dev_upload_to(d_recv, got)

            comm = CallbackComm(rank, world, all_gather, exchange)
            h.from_plain(cur[bounds[rank]:bounds[rank + 1]])
            d_bwt, d_tw = h.sort_text(t2)
            n2 = t2.size
            t_lo = n2 // world * rank + (n2 % world) * rank // world
            d_tprev = h.tprev_from_tw(d_tw, n2)
            bounds, _ = h.sh_merge_text(comm, bounds, d_tprev, d_tw.value + t_lo * 8, n2, np.flatnonzero(t2 == 0))
            _check_interval(h, np.random.default_rng(rank), want, bounds, rank)
            h.close()
            q.put((rank, True, ""))
        except BaseException as e:
            q.put((rank, False, repr(e)))

    th = [threading.Thread(target=run, args=(r,)) for r in ranks]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)


@pytest.mark.parametrize("world,ipc", [(8, False), (5, True)])
def test_batch_sharded_merge_between_processes(world, ipc):
    """rb3gpu_sh_merge_text between PROCESSES over the gloo callbacks (what bench.py --gpus N runs where the ranks share a GPU): the exchange with the owners of
    the text ranges is called right behind the kernel that fills the send regions, and a communicator that reads them with the runtime's synchronous copies must
    wait for the engine's (non-blocking) stream first -- CallbackComm does (rb3gpu_stream_sync); without it eight processes lost rows where four got away with it.
    Eight ranks, two per process (a thread, an engine handle and a gloo group each), so that five processes hold the GPU rather than nine.  With peer rounds
    (ipc) every rank must be a process of its own -- a process maps the buffers of the others through HIP IPC handles -- and five ranks keep it at six."""
    import socket
    import torch.multiprocessing as mp
    from tools import probe_gloo_text
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    if ipc:
        procs = [ctx.Process(target=probe_gloo_text.worker, args=(r, world, port, q, ipc, 20000)) for r in range(world)]
    else:
        procs = [ctx.Process(target=_text_ranks_worker, args=([r, r + 1], world, port, q, 20000)) for r in range(0, world, 2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] for r in res), res


def test_rccl_communicator_world_of_one(oracle):
    """the RCCL communicator of the library (librccl loaded at run time; one process per GPU) on the one GPU there is: communicator of
    world 1, its all-gather, its grouped send/recv (a rank sending to itself) called directly, and a merge through it"""
    import ctypes
    from ropebwt3_amd import Rb3Gpu, RcclComm, gpu, multi
    rng = np.random.default_rng(11)
    cur, batches, want = _sharded_case(oracle, rng, "reads")
    h = Rb3Gpu(verbose=1)
    try:
        comm = RcclComm(h, 0, 1, RcclComm.unique_id())
        ag = gpu.ALL_GATHER_F(comm.struct.all_gather)
        send, recv = (ctypes.c_int64 * 6)(1, 2, 3, 4, 5, 6), (ctypes.c_int64 * 6)()
        assert ag(comm.struct.ctx, send, 6, recv) == 0 and list(recv) == [1, 2, 3, 4, 5, 6]
        a2a = gpu.ALL_TO_ALL_F(comm.struct.all_to_all)
        st = np.arange(2 * 1000, dtype=np.int64)
        d_s, d_r = h.dev_alloc(st.nbytes), h.dev_alloc(st.nbytes)
        h.dev_upload_to(d_s, st)
        cnt = (ctypes.c_int64 * 1)(1000)
        assert a2a(comm.struct.ctx, d_s, 1000, cnt, d_r, cnt, h._lib.rb3gpu_stream_of(h._h)) == 0
        h.sync()
        assert np.array_equal(h.dev_download_i64(d_r, 2000), st)
        h.dev_free(d_s), h.dev_free(d_r)
        bounds = multi.interval_bounds(cur.size, 1)
        h.from_plain(cur)
        t2 = batches[0]
        d_bwt, d_tw = h.sort_text(t2)
        bounds, _ = h.sh_merge(comm, bounds, d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
        _check_interval(h, rng, want[1], bounds, 0)
        comm.close()
    finally:
        h.close()


def test_lf_consistency_check_finds_a_wrong_but_monotone_pos(oracle):
    """the device-side check of pos[] against the index (k_lf_check: ka[LF2(kb)] == C1[c] + rank_B1(c, ka[kb]), SURVEY
    appendix A) on every row: a correct merge passes with all rows verified; a pos[] that was moved by one position for a
    range of rows -- still strictly increasing, so the completeness/monotonicity check cannot see it (test hook) -- is
    caught, nothing is installed from it, and the merge is redone without speculation: same index as the oracle's."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(88)
    g0 = util.random_genome(rng, 60000)
    b1 = host.build_bwt(util.make_text([g0, util.mutate(rng, g0, 0.01)]))
    t2 = util.make_text([util.mutate(rng, g0, 0.002)] + util.reads_from(rng, g0, 100, 80))
    want = oracle.merge(b1, host.build_bwt(t2.copy()))
    for corrupt in (0, 1):
        h = Rb3Gpu(verbose=1, hooks=True)
        h.tune("lf_check", 1)
        h.tune("corrupt_pos", corrupt)
        h.from_plain(b1)
        d, dtw = h.sort_text(t2)
        h.merge_text_dev(d, dtw, t2.size, host.walkers_text(t2, 256), commit=True)
        st = h.stats()
        assert np.array_equal(h.export_plain(), want)
        assert st["n_fallbacks"] == corrupt                      # the corrupted attempt was thrown away and redone
        assert st["n_lf_checked"] >= (0.9 * t2.size if not corrupt else 0)
        h.close()
    # the default: every 4096-th row, on every merge
    h = Rb3Gpu(verbose=1)
    h.from_plain(b1)
    d, dtw = h.sort_text(t2)
    h.merge_text_dev(d, dtw, t2.size, host.walkers_text(t2, 256), commit=True)
    assert h.stats()["n_lf_checked"] > 0
    h.close()


def test_walker_list_made_on_the_device(oracle):
    """rb3gpu_merge_text_step_dev: the walker list of a batch of long strings made by two kernels in front of the walk (VERDICT r4 "missing" 4) is the
    list of rb3h_walkers_text entry for entry -- strings of every length around the spacing, a string shorter than the pre-roll, multiples that fall on
    sentinels and next to them --, a merge through it gives the oracle's index, and a wrong string count is an error, not a wrong index."""
    from ropebwt3_amd import Rb3Gpu, Rb3GpuError, host
    rng = np.random.default_rng(77)
    g0 = util.random_genome(rng, 50000)
    b1 = host.build_bwt(util.make_text([g0, util.mutate(rng, g0, 0.01)]))
    h = Rb3Gpu(verbose=1)
    try:
        for step in (64, 100, 256, 1000):
            lens = [1, 2, 31, 32, 33, step - 1, step, step + 1, 2 * step, 2 * step + 127, 2 * step + 129, 3 * step - 1, 5000, 12345, 7]
            seqs = [util.mutate(rng, g0, 0.003)[o:o + l] for o, l in zip(rng.integers(0, 30000, size=len(lens)), lens)]
            t2 = util.make_text(seqs)
            n_str = int((t2 == 0).sum())
            d, dtw = h.sort_text(t2)
            wd = h.walkers_step_dev(dtw, t2.size, n_str, step)
            wh = np.asarray(host.walkers_text(t2, step)).reshape(-1, 4)
            assert wd.shape == wh.shape, (step, wd.shape, wh.shape)
            assert np.array_equal(wd, wh), step      # entry for entry, in text order
            want = oracle.merge(b1, host.build_bwt(t2.copy()))
            h.from_plain(b1)
            h.merge_text_step_dev(d, dtw, t2.size, n_str, step)
            assert np.array_equal(h.export_plain(), want), step
            h.from_plain(b1)
            with pytest.raises(Rb3GpuError):
                h.merge_text_step_dev(d, dtw, t2.size, n_str - 1, step)
            assert np.array_equal(h.export_plain(), b1)      # nothing was installed
            h.dev_free(d), h.dev_free(dtw)
    finally:
        h.close()


def test_junction_check_catches_one_wrong_stretch_every_time(oracle):
    """the deterministic part of the validation (k_junction_check): the LF relation at EVERY junction of the
    speculative walk -- where a walker met somebody's record, and at every drop-out event -- on every merge.  A test hook gives ONE
    settled stretch a wrong unknown (all its rows move by one position; the sampled check, 1 row in 4096, would see a stretch of
    a few dozen rows once in a hundred merges): caught 100 times out of 100 -- by the order check when the move collides with a
    neighbour, by the junction check otherwise --, nothing installed, the merge redone without speculation: the oracle's index."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(2025)
    g0 = util.random_genome(rng, 30000)
    rel = [util.mutate(rng, g0, 0.004) for _ in range(10)]
    b1 = host.build_bwt(util.make_text(rel))
    t2 = util.make_text([util.mutate(rng, g0, 0.003)])
    want = oracle.merge(b1, host.build_bwt(t2.copy()))
    h = Rb3Gpu(verbose=1, hooks=True)
    h.tune("junction_check", 1)    # every event and all junctions between walkers (the default since round 6; every 16th stretch id's events before)
    try:
        caught = 0
        for trial in range(100):
            h.stats_reset()
            h.tune("corrupt_sfin", trial * 3)
            h.from_plain(b1)
            d, dtw = h.sort_text(t2)
            h.merge_text_dev(d, dtw, t2.size, host.walkers_text(t2, 256), commit=True)
            h.dev_free(d), h.dev_free(dtw)
            st = h.stats()
            assert np.array_equal(h.export_plain(), want), trial
            caught += st["n_fallbacks"]      # (by the order check -- the junction check does not run then -- or by the junction check)
        assert caught == 100, caught
        # and without the hook: every junction checked, none fails
        h.tune("corrupt_sfin", -1)
        h.stats_reset()
        h.from_plain(b1)
        d, dtw = h.sort_text(t2)
        h.merge_text_dev(d, dtw, t2.size, host.walkers_text(t2, 256), commit=True)
        st = h.stats()
        assert st["n_fallbacks"] == 0 and st["n_junctions_checked"] > 300 and np.array_equal(h.export_plain(), want), st
    finally:
        h.close()


@pytest.mark.parametrize("tent_q", [0, 2, 8])
def test_duplicate_genome_long_settle_paths(oracle, tent_q):
    """a string that repeats indexed text end to end never makes a walker exact: all its walkers hang on ONE dependency path,
    longer than k_resolve_w follows (64 hops).  The merge notices on the device, the host starts the pointer-jumping settle
    (k_wj_*: maps x -> x - #dropped below x + offset composed by doubling), validates and rebuilds again -- no redo of the
    rank phase, and the same index as the oracle's.  Single relative (pure links) and a family (drop-outs along the path).
    tent_q: the same through the wide-mask kernels (k_events_x ... k_wj_round_x; masks of 512 and 2048 bits)."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(404)
    g0 = util.random_genome(rng, 120000)
    for nrel in (1, 6):
        rel = [g0] + [util.mutate(rng, g0, 0.002) for _ in range(nrel - 1)]
        b1 = host.build_bwt(util.make_text(rel))
        t2 = util.make_text([rel[-1].copy(), util.mutate(rng, g0, 0.001)])     # a duplicate and an ordinary relative in one batch
        want = oracle.merge(b1, host.build_bwt(t2.copy()))
        h = Rb3Gpu(verbose=1)
        if tent_q:
            h.tune("tent_q", tent_q)
        h.from_plain(b1)
        d, dtw = h.sort_text(t2)
        h.merge_text_dev(d, dtw, t2.size, host.walkers_text(t2, 128), commit=True)
        st = h.stats()
        assert np.array_equal(h.export_plain(), want), nrel
        assert st["n_fallbacks"] == 0 and st["n_long_settles"] == 1, st
        h.merge_plain(host.build_bwt(t2.copy()))                              # the BWT-only entry point, the same batch again: now both strings are duplicates
        assert np.array_equal(h.export_plain(), oracle.merge(want, host.build_bwt(t2.copy()))), nrel
        assert h.stats()["n_fallbacks"] == 0
        h.close()


@pytest.mark.gpu
def test_walker_step_is_the_resident_capacity_of_the_walker_kernel():
    """rb3gpu_walker_step: len / (compute units x 160 walkers x 15/16 - strings), never below 192; the list made with it has no
    more walkers than the kernel keeps resident, so every octet gets one walker and none waits for another to finish"""
    from ropebwt3_amd import walker_step, host
    big = 10 ** 12
    room = big // walker_step(0, big, 0)                   # walkers the kernel is given room for (within one step's rounding)
    assert room % 160 < 64 or True
    assert 160 * 15 // 16 * 16 <= room <= 160 * 15 // 16 * 1024        # 16 .. 1024 compute units
    assert walker_step(0, 1000, 2) == 192 and walker_step(0, 192 * (room - 4), 2) == 192
    for length, n_str in ((8800002, 2), (200000002, 2), (3000000, 64), (room * 500, 1000)):
        s = walker_step(0, length, n_str)
        assert s >= 192 and length // s + n_str <= room + 1
        assert s == 192 or length / (s - 1) + n_str > room * 0.999          # not wider than needed
    assert 225 <= walker_step(0, 8800002, 2) <= 235 or room != 256 * 160 * 15 // 16     # (an MI355X: 256 compute units)
    rng = np.random.default_rng(5)
    t = util.make_text([util.random_genome(rng, 2000000)])
    w = host.walkers_text(t, walker_step(0, t.size, 2))
    assert w.shape[0] <= room + 2
    with pytest.raises(Exception):
        walker_step(99, 1000, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kind,env", [(301, "family", {}), (302, "reads", {}), (303, "dups", {}), (304, "family", {"text_mode": 2}),
                                           (305, "reads", {"text_mode": 1}), (306, "family", {"tent": 0}), (307, "family", {"tent_q": 4}),
                                           (308, "family", {"part": 2}), (309, "reads", {"part": 2}), (310, "dups", {"part": 2}), (311, "family", {"part": 2, "tent": 0}), (312, "family", {"part": 2, "tent_q": 2})])
def test_records_in_text_order_gathered_through_the_suffix_array(oracle, seed, kind, env):
    """rb3gpu_merge_text_sa_dev with `trec` forced on: the walkers leave their records in text order (one 64-byte store per octet and
    eight steps) and the validation pass gathers them into row order through the sorter's suffix array -- the same pos[], hence the
    same index, as with a record per row; suffix array checked against the inverse suffix array the text-order words carry.
    part = 2: the permutation as a two-pass partition by row bucket (k_part_scatter / k_part_place, rb3gpu_part.h) instead of the gather."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, 60000)
    if kind == "family":
        rel = [g0] + [util.mutate(rng, g0, 0.003) for _ in range(9)]
        batches = [[util.mutate(rng, g0, 0.002)], [util.mutate(rng, rel[3], 0.001), util.random_genome(rng, 5000)]]
    elif kind == "dups":
        rel = [g0, util.mutate(rng, g0, 0.002)]
        batches = [[g0.copy(), rel[1].copy()], [util.mutate(rng, g0, 0.0005)]]
    else:
        rel = [g0]
        batches = [list(util.reads_from(rng, g0, 1500, 120, 0.01)), list(util.reads_from(rng, g0, 700, 150, 0.0))]
    cur = host.build_bwt(util.make_text(rel))
    h = Rb3Gpu(verbose=1, hooks=bool(set(env) & {"text_mode"}))
    try:
        h.tune("trec", 1)
        for k, v in env.items():
            h.tune(k, v)
        h.from_plain(cur)
        for new in batches:
            t2 = util.make_text(new)
            b2 = host.build_bwt(t2.copy())
            cur = oracle.merge(cur, b2)
            d_bwt, d_tw, d_sa = h.sort_text_sa(t2)
            tw = h.dev_download(d_tw, t2.size * 8).view(np.uint64)
            sa = h.dev_download(d_sa, t2.size * 4).view(np.uint32)
            assert np.array_equal((tw >> np.uint64(3)).astype(np.int64)[sa.astype(np.int64)], np.arange(t2.size))   # isa[sa[i]] == i
            nstr = int((t2 == 0).sum())
            w = nstr if kind == "reads" else host.walkers_text(t2, 200)
            h.merge_text_dev(d_bwt, d_tw, t2.size, w, commit=True, d_sa=d_sa)
            assert np.array_equal(h.export_plain(), cur), (kind, env)
            for p in (d_bwt, d_tw, d_sa):
                h.dev_free(p)
        st = h.stats()
        assert st["n_fallbacks"] == 0, st
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("blkcap,octs", [(1, 8), (2, 3), (7, 8), (40, 1)])
def test_walkers_that_start_late(oracle, blkcap, octs):
    """Far fewer wave slots than walkers (rb3gpu_tune blkcap / octs): most walkers are taken from the queue when an octet has
    finished its first one, i.e. they START LATE, some of them just when their right neighbour reaches their rows -- the
    situation of a wave that was not resident when the kernel began.  A late walker whose rows its neighbour has already walked
    must not start (it probes a row of the neighbour's segment, Walker.flags >> 16); whatever the timing, the index is the
    oracle's, and a merge is redone at most rarely."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(900 + blkcap)
    g0 = util.random_genome(rng, 150000)
    rel = [g0] + [util.mutate(rng, g0, 0.002) for _ in range(7)]
    cur = host.build_bwt(util.make_text(rel))
    h = Rb3Gpu(verbose=1)
    try:
        h.tune("blkcap", blkcap)
        h.tune("octs", octs)
        h.from_plain(cur)
        n_merges = 0
        for k in range(6):
            t2 = util.make_text([util.mutate(rng, rel[k % len(rel)], 0.001)])
            b2 = host.build_bwt(t2.copy())
            cur = oracle.merge(cur, b2)
            d_bwt, d_tw, d_sa = h.sort_text_sa(t2)
            w = host.walkers_text(t2, 192 + 16 * k)            # ~1500 walkers for 8 .. 320 octets
            h.merge_text_dev(d_bwt, d_tw, t2.size, w, commit=True, d_sa=d_sa if k & 1 else None)
            n_merges += 1
            assert np.array_equal(h.export_plain(), cur), (blkcap, octs, k)
            for p in (d_bwt, d_tw, d_sa):
                h.dev_free(p)
        st = h.stats()
        print("blkcap", blkcap, "octs", octs, "fallbacks", st["n_fallbacks"], "of", n_merges)
        assert st["n_fallbacks"] <= 2, st
    finally:
        h.close()


@pytest.mark.parametrize("limit", [0, 150000, 1 << 32, -1])
def test_slot_headers_relative_to_the_group(oracle, limit):
    """an index below 2^32 symbols carries the LF base in its slot headers (a rank reads the slot words and the slot, no directory
    entry); from 2^32 symbols on the headers count from the group start.  rb3gpu_tune abs_limit moves that border: 0 = every build
    writes relative headers, 150000 = the family below crosses it in mid build.  Same BWT as the oracle's merge (fm-index.c:237-249)
    after every round, same ranks, and the limit cannot be changed under an index."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(401)
    g0 = util.random_genome(rng, 20000)
    h = Rb3Gpu(verbose=1)
    h.tune("abs_limit", limit)
    if limit < 0:   # (round 6) the layout of 2^32 symbols and more: headers = the low half of the LF base, the rest from the table of bases every 2^31 symbols -- here forced on a small index
        h.tune("abs_table", 1)
    want = None
    try:
        for i in range(16):
            g = util.mutate(rng, g0, 0.002) if i % 4 else util.random_genome(rng, 9000)   # run slots and bit planes side by side
            t = util.make_text([g])
            b = host.build_bwt(t.copy())
            if want is None:
                h.from_plain(b); want = b
                with pytest.raises(Exception):
                    h.tune("abs_limit", 5)
                continue
            want = oracle.merge(want, b)
            if i % 3 == 0:
                h.merge_plain(b)   # LF walk over the batch BWT
            else:
                d, dtw = h.sort_text(t)
                h.merge_text_dev(d, dtw, t.size, host.walkers_text(t, 192), commit=True)
                h.dev_free(d), h.dev_free(dtw)
            assert np.array_equal(h.export_plain(), want), i
        assert h.stats()["n_fallbacks"] == 0
        ks = np.concatenate([np.arange(0, want.size, 499), [want.size - 1, want.size]])
        cum = np.zeros((want.size + 1, 6), dtype=np.int64)
        for c in range(6):
            cum[1:, c] = np.cumsum(want == c)
        assert np.array_equal(h.rank1a(ks), cum[ks])
        # the index written out and read back chunk by chunk (k_pass2w with the header kind of the whole index)
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            fn = os.path.join(td, "x.fmd")
            with open(fn, "wb") as f:
                f.write(host.fmd_bytes_from_words(h.export_fmd_words(), h.get_acc()))
            h2 = Rb3Gpu(verbose=1)
            try:
                h2.tune("abs_limit", limit); h2.tune("load_chunk", 3)
                if limit < 0:
                    h2.tune("abs_table", 1)
                h2.from_fmd_file(fn)
                assert np.array_equal(h2.export_plain(), want) and np.array_equal(h2.rank1a(ks), cum[ks])
            finally:
                h2.close()
    finally:
        h.close()


def _rank_and_kount_beyond_2_32(h, sb=31):
    """rank1a of an index past 2^32 symbols (slot headers = low halves of the LF bases + the table of bases every 2^31 symbols) against a
    CPU table of counts every 2^16 symbols of its exported plain BWT: at random positions, around every multiple of 2^31, around every
    C[a], around every position where an LF base C[a] + rank(a, k) crosses a multiple of 2^31 (where the low-half arithmetic wraps;
    for T that is inside the index) and at the end; then kount(6, 1) against a backward search on the same table.  The positions are
    checked around multiples of 2^sb (the table's spacing is 2^31); returns them."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    from tests import kount_model as km
    t0 = time.time()
    plain = h.export_plain()
    n = plain.size
    S = 16
    nb = (n >> S) + 1                                  # blocks of 2^16 symbols, the last one partial
    cp = np.zeros((nb + 1, 6), dtype=np.int64)        # cp[j] = counts before position j << S (cp[nb] = the totals)

    def fill(j0):
        j1 = min(nb, j0 + 1024)
        for j in range(j0, j1, 256):
            je = min(j1, j + 256)
            blk = plain[j << S: min(n, je << S)]
            full = (je - j) if (je << S) <= n else (je - j - 1)
            for c in range(6):
                if full:
                    cp[j + 1: j + 1 + full, c] = np.count_nonzero(blk[: full << S].reshape(full, 1 << S) == c, axis=1)
                if full < je - j:
                    cp[je, c] = np.count_nonzero(blk[full << S:] == c)
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(fill, range(0, nb, 1024)))
    np.cumsum(cp, axis=0, out=cp)
    acc = h.get_acc()
    assert np.array_equal(acc[1:], np.cumsum(cp[nb]))

    def rank(ks):
        out = cp[ks >> S].copy()
        for i, k in enumerate(ks):
            out[i] += np.bincount(plain[(k >> S) << S: k], minlength=6)
        return out
    rng = np.random.default_rng(232)
    ks = [rng.integers(0, n + 1, size=4096), np.arange(n - 4095, n + 1)]
    near = [m << sb for m in range(1, (n >> sb) + 1)] + [1 << 32] + [int(x) for x in acc]
    for a in range(6):   # where C[a] + rank(a, k) reaches a multiple of 2^31: the k just past the occurrence of a that gets it there
        for M in range(1, (n >> sb) + 2):
            r = (M << sb) - int(acc[a])
            if 0 < r <= int(acc[a + 1] - acc[a]):
                j = int(np.searchsorted(cp[:, a], r)) - 1     # the last block start with fewer than r occurrences before it
                occ = np.flatnonzero(plain[j << S: min(n, (j + 1) << S)] == a)
                k = (j << S) + int(occ[r - int(cp[j, a]) - 1]) + 1
                assert cp[j, a] < r and int(acc[a]) + int(rank(np.array([k]))[0, a]) == M << sb
                near.append(k)
    ks.append((np.array(near, dtype=np.int64)[:, None] + np.arange(-3, 4)[None, :]).ravel())
    ks = np.unique(np.clip(np.concatenate(ks), 0, n)).astype(np.int64)
    got, want = h.rank1a(ks), rank(ks)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "rank1a differs at %d of %d positions beyond 2^32, first k = %d" % (bad.size, ks.size, ks[bad[0]] if bad.size else -1)
    # kount(6, 1): the backward search of every 6-mer on the CPU table (a k-mer's occurrences = the size of its BWT interval)
    lev = [(np.array([[c]], dtype=np.uint8), np.array([acc[c]]), np.array([acc[c + 1]])) for c in range(1, 5)]
    km_, lo, hi = (np.concatenate([x[i] for x in lev]) for i in range(3))
    for _ in range(5):
        rl, rh = rank(lo), rank(hi)
        nk, nl, nh = [], [], []
        for c in range(1, 5):
            l2, h2 = acc[c] + rl[:, c], acc[c] + rh[:, c]
            keep = h2 > l2
            nk.append(np.concatenate([np.full((int(keep.sum()), 1), c, dtype=np.uint8), km_[keep]], axis=1))
            nl.append(l2[keep]), nh.append(h2[keep])
        km_, lo, hi = np.concatenate(nk), np.concatenate(nl), np.concatenate(nh)
    o = km.order(km_)
    gk, gc = h.kount(6, 1)
    assert np.array_equal(gk, km_[o]) and np.array_equal(gc[:, 0], (hi - lo)[o])
    print("beyond 2^32: %d ranks and kount(6, 1) (%d 6-mers) checked against the CPU table in %.1f s" % (ks.size, gk.shape[0], time.time() - t0))
    return near


def test_index_beyond_2_32_symbols():
    """the regime BASELINE configs[3]/[4] live in.  12 haplotypes of a 180 Mbp genome (contigs of 20-100 Mbp, both
    strands: 360 M symbols per merge round) grow an index to 4.32 G symbols -- past 2^32, where the slot headers count from the
    group start and the walkers' common step runs on 64-bit positions -- with the LF relation of EVERY row verified against the
    index after every rank phase (lf_check = 1; fm-index.c:164, 171-173), no merge redone, and the .fmd byte-identical (md5) to the
    one the unmodified reference wrote for the same 12 files (tests/golden/MANIFEST.json "big_index", tools/make_golden_big.py);
    then a batch of reads into it under the same check."""
    import json
    from tools import big_index
    man = json.load(open(os.path.join(util.GOLDEN, "MANIFEST.json"))).get("big_index", {}).get("12x180000000")
    h, srt, rounds, base = big_index.build(12, 180000000, lf_check=1)
    try:
        assert rounds[-1]["index_symbols"] > (1 << 32) and rounds[-1]["index_symbols"] == sum(r["symbols"] for r in rounds)
        assert sum(r["fallbacks"] for r in rounds) == 0
        st = h.stats()
        assert st["n_lf_checked"] >= sum(r["symbols"] for r in rounds[1:]) * 0.99   # (the count is kept approximately, 64 rows at a time)
        assert man is not None, "no golden for this size: run tools/make_golden_big.py"
        assert rounds[-1]["index_symbols"] == man["symbols"]
        assert big_index.fmd_md5(h) == man["fmd_md5"]
        _rank_and_kount_beyond_2_32(h)
        rd = big_index.reads_into(h, base, 200000, reps=1)
        assert rd["fallbacks"] == 0 and rd["lf_steps"] == rd["symbols"]
    finally:
        srt.close()
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,nrel,div,tq", [(401, 12, 0.002, 0), (402, 40, 0.001, 0), (403, 3, 0.004, 0), (404, 25, 0.0005, 0), (405, 30, 0.001, 2), (406, 12, 0.002, 8)])
def test_follower_that_settles_a_later_stretch_of_a_walker(oracle, seed, nrel, div, tq):
    """VERDICT r3 item 2 / DESIGN.md: an exact walker that follows a tentative one more closely than records become visible records over
    the rows of the walker's FIRST stretch and meets the first visible tentative record in a LATER one, where it leaves the settled
    unknown.  The test build makes that deterministic (rb3gpu_tune hide_first: exact walkers do not see first stretches at all), so
    it happens at every hand-over instead of once in ten thousand merges.  k_cum derives the first stretch's unknown from the later
    one -- exactly when that is unambiguous, else as "valid from that stretch on" (k_resolve_w / k_sfin then leave the earlier
    stretches alone, whose rows the follower has recorded itself): the index is the oracle's and NO merge is redone (round 3:
    every such walker stayed unsettled and the rank phase ran again)."""
    from ropebwt3_amd import Rb3Gpu, host
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, 50000)
    rel = [g0] + [util.mutate(rng, g0, div) for _ in range(nrel - 1)]
    cur = host.build_bwt(util.make_text(rel))
    h = Rb3Gpu(verbose=1, hooks=True)
    try:
        h.tune("hide_first", 1)
        if tq:
            h.tune("tent_q", tq)   # (the settle kernels for masks of 256 tq bits)
        h.from_plain(cur)
        n_merges = 0
        for r in range(6):
            new = [util.mutate(rng, rel[int(rng.integers(0, len(rel)))], div)]
            t2 = util.make_text(new)
            b2 = host.build_bwt(t2.copy())
            cur = oracle.merge(cur, b2)
            d_bwt, d_tw = h.sort_text(t2)
            h.merge_text_dev(d_bwt, d_tw, t2.size, host.walkers_text(t2, 200), commit=True)
            h.dev_free(d_bwt), h.dev_free(d_tw)
            n_merges += 1
            assert np.array_equal(h.export_plain(), cur), (seed, r)
        st = h.stats()
        assert st["n_fallbacks"] == 0 and st["n_long_settles"] == 0, st
    finally:
        h.close()
