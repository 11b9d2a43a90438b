"""fetch on the GPU: Rb3Gpu.fetch against the indexed records and the model (tests/fetch_model.py), its statistics included, at five sample rates, two slice
budgets, on a merged index and with the samples uploaded from the host; the refusals of the engine; random access (the steps of a short region at the start of a
long string); the command line on every kind of index, with BED, --row and -s, and its refusals; the pipeline sw -> fetch; the live reference's `get`."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError
from tests import fetch_model as fm
from tests import kount_model as km
from tests import util

CLI = _build.BIN_CLI
GOLDEN = util.GOLDEN
EINVAL, ESTATE, EINTERNAL = -3, -5, -6          # include/rb3gpu.h
MSG = b"ERROR: failed to load suffix array samples or sequence names/lengths\n"
NT6 = {c: i for i, c in enumerate("$ACGTN")}


def _run(args, env=None, timeout=120):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)


def _random_records(seed, n_genomes=4, length=2500):
    """the records of the get tests: relatives of one genome, a record with N and a repeat, records of one and two symbols"""
    rng = np.random.default_rng(seed)
    g0 = util.random_genome(rng, length)
    recs = [g0] + [util.mutate(rng, g0, 0.02) for _ in range(n_genomes - 1)]
    recs.append(np.concatenate([g0[100:400], np.full(3, 5, dtype=np.uint8), g0[:200]]))
    recs.append(g0[:1].copy())
    recs.append(g0[7:9].copy())
    return rng, recs


def _strands(recs):
    out = []
    for s in recs:
        out += [np.asarray(s, dtype=np.uint8), util.revcomp(np.asarray(s, dtype=np.uint8))]
    return out


_REF = {}


def _reference():
    """the records, their strands, the BWT of the index and per sample rate the model and the regions with the model's answers: computed once, shared, never
    changed"""
    if not _REF:
        rng, recs = _random_records(4)
        _REF.update(recs=recs, strings=_strands(recs), bwt=host.build_bwt(util.make_text(recs)), oracle=util.Oracle(), rng=rng, at={})
    return _REF


def _at(S):
    R = _reference()
    if S not in R["at"]:
        ms, r2i, ssa = R["oracle"].ssa_gen(R["bwt"], S)
        model = fm.FetchModel(R["bwt"], S, ms, r2i, ssa)
        strings = R["strings"]
        rng = np.random.default_rng(100 + S)
        regions, kinds = [], set()
        for r, s in enumerate(strings):
            for kind, reg in fm.edge_regions(model, r, len(s)).items():
                kinds.add(kind)
                regions.append(reg)
        for _ in range(2000):                                          # random regions, most of them short, some up to the whole string
            r = int(rng.integers(0, len(strings)))
            n = len(strings[r])
            ln = int(min(n, rng.integers(1, 65) if rng.random() < 0.9 else rng.integers(1, n + 1)))
            beg = int(rng.integers(0, n - ln + 1))
            regions.append((r, beg, beg + ln))
        regions += regions[5:15] + [(0, 100, 300), (0, 200, 400), (0, 150, 250), (0, 100, 300)]     # duplicates and overlaps
        seqs, st = model.fetch(regions)
        assert all(np.array_equal(g, strings[r][b:e]) for g, (r, b, e) in zip(seqs, regions))
        R["at"][S] = dict(model=model, regions=regions, kinds=kinds, seqs=seqs, st=st, ms=ms, r2i=r2i, ssa=ssa)
    return R["at"][S]


def _fetch(h, regions, stats=True):
    a = np.array(regions, dtype=np.int64).reshape(-1, 3)
    return h.fetch(a[:, 0], a[:, 1], a[:, 2], stats=stats)


def _eq(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


STAT_KEYS = ("n_walkers", "n_measured", "n_steps", "max_walk_steps")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [0, 1, 3, 8, 20])
def test_api_matches_records_and_model(S):
    """the symbols are the records' and the walkers, measured regions, steps and the longest walk are the model's, whatever the slices.  At S = 20 only row m
    is a sample: nearly every region is measured, most strings have no sample at all"""
    R, A = _reference(), _at(S)
    missing = set(fm.EDGE_KINDS) - A["kinds"]
    # (S = 0: every offset of a string is a sample, none lies between or beyond samples; S = 20: one sample in the whole index)
    assert missing <= ({"between_samples", "beyond_last_sample"} if S == 0 else {"beg_at_sample", "end_at_sample", "end_above_sample", "between_samples"} if S == 20 else set()), missing
    if S == 20:
        assert len(A["ssa"]) == 1 and A["st"]["n_measured"] > len(A["regions"]) * 0.8
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(R["bwt"])
        h.keep_ssa(S)
        seqs, st = _fetch(h, A["regions"])
        print(S, {k: st[k] for k in STAT_KEYS}, {k: A["st"][k] for k in STAT_KEYS})
        assert _eq(seqs, A["seqs"])
        assert {k: st[k] for k in STAT_KEYS} == {k: A["st"][k] for k in STAT_KEYS}
        assert st["n_regions"] == len(A["regions"]) and st["n_symbols"] == sum(e - b for _, b, e in A["regions"]) and st["n_slices"] == 1 and st["ms_table"] > 0
        for budget in (64, 50000):                                   # most regions a slice of their own, some longer than the budget; a few slices
            h.tune("fetch_slice", budget)
            seqs, st2 = _fetch(h, A["regions"])
            assert _eq(seqs, A["seqs"]) and {k: st2[k] for k in STAT_KEYS} == {k: A["st"][k] for k in STAT_KEYS}
            assert st2["n_slices"] > (len(A["regions"]) // 4 if budget == 64 else 1) and st2["ms_table"] == 0      # (the table is kept)
        assert _fetch(h, [], stats=False) == []
    finally:
        h.close()


@pytest.mark.gpu
def test_api_on_a_merged_index_with_uploaded_samples():
    R, A = _reference(), _at(3)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(host.build_bwt(util.make_text(R["recs"][:3])))
        h.merge_plain(host.build_bwt(util.make_text(R["recs"][3:])))
        ms, r2i, ssa = h.ssa_gen(3)
        assert ms == A["ms"] and np.array_equal(ssa, A["ssa"])
        h.set_ssa(3, ms, r2i, ssa)
        seqs, st = _fetch(h, A["regions"])
        assert _eq(seqs, A["seqs"]) and {k: st[k] for k in STAT_KEYS} == {k: A["st"][k] for k in STAT_KEYS}
    finally:
        h.close()


@pytest.mark.gpu
def test_api_refusals():
    R, A = _reference(), _at(8)
    model, strings = A["model"], R["strings"]
    m = len(strings)
    good = [(0, 10, 90), (3, 0, len(strings[3])), (11, 0, 1)]
    no_anchor = [r for r in range(m) if len(strings[r]) > 100 and model.plan(r, 5, len(strings[r]))[2] is None][0]
    h = Rb3Gpu(verbose=0)
    try:
        h.from_plain(R["bwt"])
        end0, seq0 = h.retrieve(range(m))
        with pytest.raises(Rb3GpuError) as e:
            _fetch(h, good)
        assert e.value.code == ESTATE                                                      # no sampled suffix array
        h.keep_ssa(8)
        want = model.fetch(good)[0]
        assert _eq(_fetch(h, good, stats=False), want)
        called = []
        for bad in [(no_anchor, 5, len(strings[no_anchor]) + 1), (0, -1, 5), (0, 7, 7), (m, 0, 1), (-1, 0, 1)]:
            with pytest.raises(fm.FetchInvalid):
                model.fetch([bad])
            for at in (0, 2, 3):
                regs = good[:at] + [bad] + good[at:] + [(m + 5, 0, 1)]
                with pytest.raises(Rb3GpuError) as e:
                    _fetch(h, regs)
                assert e.value.code == EINVAL and e.value.bad == at and "region %d" % at in str(e.value), (bad, at)
        # the callback is never called for a request with an invalid region: straight at the C entry point
        import ctypes
        from ropebwt3_amd import gpu

        def cb(*_a):
            called.append(1)
            return 0
        reg = np.array(good + [(0, 7, 7)], dtype=np.int64)
        bad = ctypes.c_int64(-5)
        assert h._lib.rb3gpu_fetch(h._h, 4, reg.ctypes.data, ctypes.byref(bad), gpu.FETCH_F(cb), None, None) == EINVAL and bad.value == 3 and not called
        assert h._lib.rb3gpu_fetch(h._h, 3, reg.ctypes.data, ctypes.byref(bad), gpu.FETCH_F(0), None, None) == EINVAL                   # a NULL callback
        assert h._lib.rb3gpu_fetch(h._h, 3, reg.ctypes.data, None, gpu.FETCH_F(lambda *_a: 7), None, None) == 7                          # the callback's own code
        assert h._lib.rb3gpu_fetch(h._h, 0, None, None, gpu.FETCH_F(cb), None, None) == 0 and not called
        assert _eq(_fetch(h, good, stats=False), want)
        h.drop_ssa()
        with pytest.raises(Rb3GpuError) as e:
            _fetch(h, good)
        assert e.value.code == ESTATE
        # the samples of another index of the same dimensions
        rng = np.random.default_rng(77)
        other = [rng.permutation(s) if len(s) > 2 else s for s in R["recs"]]
        ob = host.build_bwt(util.make_text(other))
        oms, or2i, ossa = R["oracle"].ssa_gen(ob, 3)
        assert ob.size == R["bwt"].size and oms == A["ms"]
        try:
            h.set_ssa(3, oms, or2i, ossa)
        except Rb3GpuError as e2:
            assert e2.code == EINVAL                                                       # (another count of sentinels or symbols: not the case here)
        else:
            with pytest.raises(Rb3GpuError) as e:
                _fetch(h, [(r, 0, len(s)) for r, s in enumerate(strings)])
            assert e.value.code == EINTERNAL
        # the handle as it was
        h.keep_ssa(8)
        assert _eq(_fetch(h, good, stats=False), want)
        end1, seq1 = h.retrieve(range(m))
        assert np.array_equal(end0, end1) and _eq(seq0, seq1)
    finally:
        h.close()
    h = Rb3Gpu(verbose=0)
    try:
        with pytest.raises(Rb3GpuError) as e:
            _fetch(h, good)
        assert e.value.code == ESTATE                                                      # no index
    finally:
        h.close()


@pytest.mark.gpu
def test_random_access_is_real():
    """100 symbols at the start of a string of more than 250 k: the steps are the model's, fewer than 100 + the offset of the region's anchor as the sampled suffix array
    itself gives it, while `get` of the same string walks all of it"""
    bwt = km.golden_plain(GOLDEN, "longruns.fmd", CLI)
    ms, r2i, ssa = util.Oracle().ssa_gen(bwt, 8)
    model = fm.FetchModel(bwt, 8, ms, r2i, ssa)
    offs = sorted(int(x) >> ms for x in ssa if int(x) & ((1 << ms) - 1) == 0)            # the samples of string 0, from the array
    anchor = min(o for o in offs if o >= 100)
    want, mst = model.fetch([(0, 0, 100)])
    assert mst["n_steps"] == anchor and mst["n_measured"] == 0
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(bwt)
        h.keep_ssa(8)
        got, st = _fetch(h, [(0, 0, 100)])
        gst = {}
        end, seqs = h.retrieve([0], stats=gst)
        assert _eq(got, want) and np.array_equal(got[0], seqs[0][:100])
        assert st["n_steps"] == mst["n_steps"] and st["n_steps"] < 100 + anchor and st["n_walkers"] == mst["n_walkers"]
        assert gst["n_steps"] >= len(seqs[0]) >= 250000                          # (string 0 of longruns has 700 000 symbols)
    finally:
        h.close()


# ---- the command line ------------------------------------------------------------------------------------------------

def _fasta(path):
    names, seqs = [], []
    for line in gzip.open(path, "rt"):
        if line.startswith(">"):
            names.append(line[1:].split()[0])
            seqs.append([])
        else:
            seqs[-1].append(line.strip())
    return names, ["".join(s).upper() for s in seqs]


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """genomes12.fmd with its .ssa (the committed one, -s8) and .len.gz side by side under the names the command expects"""
    d = tmp_path_factory.mktemp("fetch")
    loc = str(d / "genomes12.fmd")
    shutil.copy(os.path.join(GOLDEN, "genomes12.fmd"), loc)
    shutil.copy(os.path.join(GOLDEN, "genomes12.s8.ssa"), loc + ".ssa")
    shutil.copy(os.path.join(GOLDEN, "genomes12.len.gz"), loc + ".len.gz")
    return loc


def _cli_regions():
    """forward and reverse regions of all 12 names: (word, BED line, --row word, the letters)"""
    names, seqs = _fasta(os.path.join(GOLDEN, "genomes12.fa.gz"))
    rng = np.random.default_rng(5)
    out = []
    for i, (nm, s) in enumerate(zip(names, seqs)):
        n = len(s)
        for beg, end in [(0, 1), (n - 1, n), (0, n), (int(rng.integers(0, n - 300)),) * 2]:
            if beg == end:
                end = beg + int(rng.integers(1, 300))
            out.append(("%s:%d-%d" % (nm, beg, end), "%s\t%d\t%d\n" % (nm, beg, end), "%d:%d-%d" % (2 * i, beg, end), s[beg:end]))
            out.append(("%s:%d-%d:-" % (nm, beg, end), "%s\t%d\t%d\tx\t0\t-\n" % (nm, beg, end), "%d:%d-%d" % (2 * i + 1, n - end, n - beg), _rc(s[beg:end])))
            out.append(("%s:%d-%d:+" % (nm, beg, end), "%s\t%d\t%d\tx\t0\t+\n" % (nm, beg, end), "%d:%d-%d" % (2 * i, beg, end), s[beg:end]))
    return out


def _expect(labels, regs):
    return "".join(">%s\n%s\n" % (l, r[3]) for l, r in zip(labels, regs)).encode()


@pytest.mark.gpu
def test_cli_matches_the_records(staged, tmp_path):
    regs = _cli_regions()
    words = [r[0] for r in regs]
    want = _expect(words, regs)
    r = _run([CLI, "fetch", staged] + words)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode(errors="replace")[-2000:]
    env = dict(os.environ, RB3GPU_FETCH_SLICE="1000")
    r = _run([CLI, "fetch", staged] + words, env=env)
    assert r.returncode == 0 and r.stdout == want and b"slice" in r.stderr and b" 1 slice(s)" not in r.stderr
    # BED: the header is name:beg-end[:strand]; half of the regions as words in front of it
    bed = tmp_path / "r.bed"
    bed.write_text("# a comment\n" + "".join(x[1] for x in regs[40:]))
    r = _run([CLI, "fetch", "-f", str(bed), staged] + words[:40])
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode(errors="replace")[-2000:]
    # --row: only the .ssa is needed
    rows = [x[2] for x in regs]
    d = tmp_path / "rowonly"
    d.mkdir()
    shutil.copy(staged, str(d / "g.fmd"))
    shutil.copy(staged + ".ssa", str(d / "g.fmd.ssa"))
    r = _run([CLI, "fetch", "--row", str(d / "g.fmd")] + rows)
    assert r.returncode == 0 and r.stdout == _expect(rows, regs), r.stderr.decode(errors="replace")[-2000:]
    # no .ssa: -s8 makes the samples on the device
    os.remove(str(d / "g.fmd.ssa"))
    r = _run([CLI, "fetch", "--row", "-s8", str(d / "g.fmd")] + rows)
    assert r.returncode == 0 and r.stdout == _expect(rows, regs), r.stderr.decode(errors="replace")[-2000:]
    shutil.copy(staged + ".len.gz", str(d / "g.fmd.len.gz"))
    r = _run([CLI, "fetch", "-s8", str(d / "g.fmd")] + words)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode(errors="replace")[-2000:]
    r = _run([CLI, "fetch", str(d / "g.fmd")] + words)
    assert r.returncode == 1 and r.stderr == MSG and r.stdout == b""


@pytest.mark.gpu
def test_cli_on_fmr_and_bre(staged, tmp_path):
    regs = _cli_regions()
    # a BRE file of the same index, made on the device
    bre = str(tmp_path / "genomes12.bre")
    r = _run([CLI, "build", "-e", "-o", bre, "-i", staged])
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-1000:]
    shutil.copy(staged + ".ssa", bre + ".ssa")
    shutil.copy(staged + ".len.gz", bre + ".len.gz")
    r = _run([CLI, "fetch", bre] + [x[0] for x in regs])
    assert r.returncode == 0 and r.stdout == _expect([x[0] for x in regs], regs), r.stderr.decode(errors="replace")[-2000:]
    # the FMR of the first six genomes: rows and names are those of the twelve
    fmr = str(tmp_path / "first6.fmr")
    shutil.copy(os.path.join(GOLDEN, "genomes12_first6.fmr"), fmr)
    r = _run([CLI, "ssa", "-s8", "-o", fmr + ".ssa", fmr])
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-1000:]
    with gzip.open(os.path.join(GOLDEN, "genomes12.len.gz"), "rt") as f:
        lines = f.readlines()[:6]
    with gzip.open(fmr + ".len.gz", "wt") as f:
        f.writelines(lines)
    six = [x for x in regs if int(x[2].split(":")[0]) < 12]
    assert len(six) == len(regs) // 2
    r = _run([CLI, "fetch", fmr] + [x[0] for x in six])
    assert r.returncode == 0 and r.stdout == _expect([x[0] for x in six], six), r.stderr.decode(errors="replace")[-2000:]
    r = _run([CLI, "fetch", "--row", fmr] + [x[2] for x in six])
    assert r.returncode == 0 and r.stdout == _expect([x[2] for x in six], six), r.stderr.decode(errors="replace")[-2000:]


@pytest.mark.gpu
def test_cli_refusals(staged, tmp_path):
    bed = tmp_path / "bad.bed"
    bed.write_text("seq1\t5\t3\n")
    nolen = tmp_path / "nolen"
    nolen.mkdir()
    shutil.copy(staged, str(nolen / "g.fmd"))
    shutil.copy(staged + ".ssa", str(nolen / "g.fmd.ssa"))
    other = tmp_path / "other"
    other.mkdir()
    shutil.copy(staged, str(other / "g.fmd"))
    shutil.copy(os.path.join(GOLDEN, "k3_both.s0.ssa"), str(other / "g.fmd.ssa"))
    shutil.copy(staged + ".len.gz", str(other / "g.fmd.len.gz"))
    fwd = tmp_path / "fwd"
    fwd.mkdir()
    shutil.copy(os.path.join(GOLDEN, "reads_fwd.fmd"), str(fwd / "r.fmd"))
    shutil.copy(os.path.join(GOLDEN, "reads_fwd.s3.ssa"), str(fwd / "r.fmd.ssa"))
    for args, line in [
        ([staged, "seq1:5-9", "seq1"], b"is no region"),                         # a word that is no region
        ([staged, "seq1:5-9", "seq1:9"], b"is no region"),
        ([staged, "seq1:-5-9"], b"is no region"),
        ([staged, "seq1:5-9:x"], b"is no region"),
        ([staged, "nobody:5-9"], b"no sequence 'nobody'"),                        # an unknown name
        ([staged, "seq1:9-9"], b"is no region"),                                  # beg >= end
        ([staged, "seq1:9-5"], b"is no region"),
        (["-f", str(bed), staged], b"is no region"),
        ([staged, "seq1:0-20001"], b"ends beyond its sequence"),                  # end beyond the sequence, by .len.gz
        ([staged, "seq1:0-20001:-"], b"ends beyond its sequence"),
        (["--row", staged, "0:0-20001"], b"lies outside the index"),              # ... and by the engine
        (["--row", staged, "24:0-1"], b"lies outside the index"),
        (["--row", staged, "seq1:0-1"], b"is no region row:beg-end"),
        (["--row", staged, "1:0-1:-"], b"is no region row:beg-end"),
        ([staged], b"no region to fetch"),                                        # no region at all
        ([str(nolen / "g.fmd"), "seq1:0-5"], MSG),                                # no .len.gz
        ([str(other / "g.fmd"), "seq1:0-5"], MSG),                                # the .ssa of another index
        ([str(fwd / "r.fmd"), "seq1:0-5"], MSG),                                  # no .len.gz beside a forward-only index
    ]:
        r = _run([CLI, "fetch"] + args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1 and r.stderr.startswith(b"ERROR: ") and line.strip() in r.stderr, (args, r.stderr)
    # a forward-only index serves --row
    reads = [x.strip() for x in gzip.open(os.path.join(GOLDEN, "reads_fwd.txt.gz"), "rt") if x.strip()]
    r = _run([CLI, "fetch", "--row", str(fwd / "r.fmd"), "0:0-%d" % len(reads[0]), "999:3-40"])
    assert r.returncode == 0 and r.stdout == (">0:0-%d\n%s\n>999:3-40\n%s\n" % (len(reads[0]), reads[0], reads[999][3:40])).encode()


@pytest.mark.gpu
def test_pipeline_sw_then_fetch(staged):
    """sw -e --seq -p1 prints the target's symbols of every hit as rs:Z:, in the QUERY's orientation: on a `-` line that is the reverse complement of the forward
    slice [column 8, column 9) of the target (established from genomes12.fa.gz below, before anything is fetched) -- which is what fetch name:beg-end:- prints"""
    names, seqs = _fasta(os.path.join(GOLDEN, "genomes12.fa.gz"))
    r = _run([CLI, "sw", "-e", "--seq", "-p1", staged, os.path.join(GOLDEN, "sw_reads.fa")])
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    hits = [x.split("\t") for x in r.stdout.decode().split("\n") if x and x.split("\t")[5] != "*"]
    minus = [x for x in hits if x[4] == "-"]
    assert len(minus) == 446 and len(hits) > len(minus)
    rs = [[t for t in x if t.startswith("rs:Z:")][0][5:] for x in hits]
    for x, t in zip(hits, rs):
        fwd = seqs[names.index(x[5])][int(x[7]):int(x[8])]
        assert t == (fwd if x[4] == "+" else _rc(fwd)) and (x[4] == "+" or t != fwd or fwd == _rc(fwd))
    words = ["%s:%s-%s:%s" % (x[5], x[7], x[8], x[4]) for x in hits]
    f = _run([CLI, "fetch", staged] + words)
    assert f.returncode == 0, f.stderr.decode(errors="replace")[-2000:]
    assert f.stdout == "".join(">%s\n%s\n" % (w, t) for w, t in zip(words, rs)).encode()


@pytest.mark.gpu
def test_cli_matches_live_reference_get(tmp_path):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    idx = os.path.join(GOLDEN, "edge_dups.fmd")
    m = int((km.golden_plain(GOLDEN, "edge_dups.fmd", CLI) == 0).sum())                   # its strings: the rows of the sentinels
    ref = _run([util.REF_BIN, "get", idx] + [str(r) for r in range(m)])
    assert ref.returncode == 0
    lines = ref.stdout.decode().split("\n")
    recs = [(int(lines[i][1:].split()[0]), lines[i + 1]) for i in range(0, len(lines) - 1, 2)]
    assert m == 12 and [r for r, _ in recs] == list(range(m))
    words = ["%d:0-%d" % (r, len(s)) for r, s in recs if len(s) > 0]
    assert len(words) >= m - 2
    loc = str(tmp_path / "edge_dups.fmd")
    shutil.copy(idx, loc)
    f = _run([CLI, "fetch", "--row", "-s3", loc] + words)
    assert f.returncode == 0, f.stderr.decode(errors="replace")[-2000:]
    assert f.stdout == "".join(">%s\n%s\n" % (w, s) for w, (r, s) in zip(words, [x for x in recs if len(x[1]) > 0])).encode()
