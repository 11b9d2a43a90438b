"""fetch without a GPU: the model (tests/fetch_model.py) against the committed indexes, their sampled suffix arrays and the records they were built from; the
model's step counts; the recorded `rs:Z:` tags of the reference's sw; the region parser of the host library; the library's symbol, the statistics' layout
and the command's usage."""
import ctypes
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, host
from tests import fetch_model as fm
from tests import util

CLI = _build.BIN_CLI
GOLDEN = util.GOLDEN
NT6 = {c: i for i, c in enumerate("$ACGTN")}


def _codes(s):
    return np.array([NT6.get(c, 5) for c in s.upper()], dtype=np.uint8)


def _fasta(path):
    names, seqs = [], []
    for line in gzip.open(path, "rt"):
        if line.startswith(">"):
            names.append(line[1:].split()[0])
            seqs.append([])
        else:
            seqs[-1].append(line.strip())
    return names, [_codes("".join(s)) for s in seqs]


def _lines(path):
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        return [_codes(x.strip()) for x in f if x.strip()]


_CASES = {}


def _case(name):
    """(model, the indexed strings in `get` order): computed once, shared, never changed"""
    if name not in _CASES:
        g = lambda f: os.path.join(GOLDEN, f)
        if name == "genomes12":
            recs, both, bwt, ssa = _fasta(g("genomes12.fa.gz"))[1], True, "genomes12.bwt.gz", "genomes12.s8.ssa"
        elif name == "k3_both":
            recs, both, bwt, ssa = _lines(g("k3_both.txt")), True, "k3_both.bwt.gz", "k3_both.s0.ssa"
        else:
            recs, both, bwt, ssa = _lines(g("reads_fwd.txt.gz")), False, "reads_fwd.bwt.gz", "reads_fwd.s3.ssa"
        strings = []
        for s in recs:
            strings += [s, util.revcomp(s)] if both else [s]
        _CASES[name] = (fm.FetchModel(fm.read_bwt(g(bwt)), *fm.read_ssa(g(ssa))), strings)
    return _CASES[name]


@pytest.mark.parametrize("name", ["genomes12", "k3_both", "reads_fwd"])
def test_model_matches_the_records(name):
    """the regions the issue names, on every string (the first 40 of the reads): the symbols are slices of the records, and the steps of the call are the
    sum of o_anchor - beg plus the measuring steps"""
    model, strings = _case(name)
    assert model.m == len(strings)
    found, regions, want = set(), [], []
    for r, s in list(enumerate(strings))[:40]:
        for kind, reg in fm.edge_regions(model, r, len(s)).items():
            found.add(kind)
            regions.append(reg)
            want.append(s[reg[1]:reg[2]])
    missing = set(fm.EDGE_KINDS) - found
    # with every row a sample (S = 0) no two samples of a string lie apart and none of its offsets is beyond the last one but the sentinel's
    assert missing <= ({"between_samples", "beyond_last_sample"} if model.S == 0 else set()), missing
    got, st = model.fetch(regions)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    measuring = sum(model.measure(r)[1] for (r, beg, end) in regions if model.plan(r, beg, end)[2] is None)
    assert st["n_steps"] == sum(o - reg[1] for o, reg in zip(st["anchor_offsets"], regions)) + measuring
    assert st["n_measured"] == sum(1 for (r, beg, end) in regions if model.plan(r, beg, end)[2] is None)
    assert st["n_walkers"] == sum(1 + len([o for o in model.samples_of(r) if beg < o < end]) for (r, beg, end) in regions)
    if model.S == 0:
        assert st["max_walk_steps"] == 1 and st["n_measured"] == len([1 for reg in regions if reg[2] == len(strings[reg[0]])])
    else:
        assert st["n_measured"] > 0 and st["max_walk_steps"] > 1


def test_model_every_row_a_sample():
    """S = 0: every walker takes exactly one step, whatever the region"""
    model, strings = _case("k3_both")
    regions = [(r, b, e) for r, s in enumerate(strings) for b in range(len(s)) for e in range(b + 1, len(s) + 1)]
    got, st = model.fetch(regions)
    assert all(np.array_equal(g, strings[r][b:e]) for g, (r, b, e) in zip(got, regions))
    assert st["max_walk_steps"] == 1 and st["n_walkers"] == sum(e - b for _, b, e in regions)
    assert st["n_steps"] == st["n_walkers"] + st["n_measured"]            # (a measuring walk is one step as well: the first row it lands on is a sample's)


def test_model_refuses_what_the_engine_refuses():
    model, strings = _case("genomes12")
    n = len(strings[3])
    top = model.samples_of(3)[-1]
    assert top + 1 < n
    for bad in [(3, 5, n + 1), (3, -1, 4), (3, 4, 4), (3, 9, 2), (model.m, 0, 1), (-1, 0, 1)]:
        with pytest.raises(fm.FetchInvalid) as e:
            model.fetch([(0, 0, 10), bad, (model.m, 0, 1)])
        assert e.value.bad == 1
    # a sampled suffix array that is not this index's: the walkers notice
    S, ms, r2i, ssa = fm.read_ssa(os.path.join(GOLDEN, "genomes12.s8.ssa"))
    other = fm.FetchModel(fm.read_bwt(os.path.join(GOLDEN, "genomes12.bwt.gz")), S, ms, r2i, np.roll(ssa, 1))
    with pytest.raises(fm.FetchInconsistent):
        other.fetch([(r, 0, len(s)) for r, s in enumerate(strings)])


def test_recorded_rs_tags_are_fetches():
    """the reference's sw --seq prints the target's symbols of every hit (rs:Z:): for the committed answer they are the model's fetch of columns 6, 8 and 9"""
    model, strings = _case("genomes12")
    names = _fasta(os.path.join(GOLDEN, "genomes12.fa.gz"))[0]
    out = json.load(open(os.path.join(GOLDEN, "SW_STDOUT.json")))["-s8 -e -u --seq -m10 genomes12.fmd mem_iupac.fa"]
    hits = [x.split("\t") for x in out.split("\n") if x and x.split("\t")[5] != "*"]
    assert len(hits) == 11 and all(x[4] == "+" for x in hits)
    regions = [(2 * names.index(x[5]), int(x[7]), int(x[8])) for x in hits]
    got, _ = model.fetch(regions)
    for x, g in zip(hits, got):
        rs = [t for t in x if t.startswith("rs:Z:")]
        assert len(rs) == 1 and rs[0][5:] == util.sym_str(g)


def test_region_parser():
    p = host.region_parse
    assert p("seq1:0-10") == (b"seq1", 0, 10, 1)
    assert p("seq1:5-6:+") == (b"seq1", 5, 6, 1) and p("seq1:5-6:-") == (b"seq1", 5, 6, -1)
    assert p("chr:1:2:7-9") == (b"chr:1:2", 7, 9, 1) and p("a:b:7-9:-") == (b"a:b", 7, 9, -1)          # the name is cut at the last colons
    assert p("x:+:3-4") == (b"x:+", 3, 4, 1) and p("n-1:3-4") == (b"n-1", 3, 4, 1)
    assert p("s:0-4611686018427387903") == (b"s", 0, (1 << 62) - 1, 1)
    for bad in ["", "seq1", "seq1:", "seq1:5", "seq1:5-", "seq1:-5", "seq1:5-5", "seq1:6-5", "seq1:-3-5", "seq1:3--5", "seq1:3-5x", "seq1:3-5:", "seq1:3-5:*",
                "seq1:3-5:+-", "seq1:3-5 ", " seq1:3 -5", ":3-5", "seq1:3-5-7", "seq1:0x3-5", "seq1:3-99999999999999999999", "seq1:99999999999999999999-3",
                "seq1:3-4611686018427387904000", "seq1:1e3-2000", "seq1:+", "3-5"]:
        assert p(bad) is None, bad
    assert p("seq1\t3\t9\n", bed=True) == (b"seq1", 3, 9, 1)
    assert p("seq1\t3\t9", bed=True) == (b"seq1", 3, 9, 1)
    assert p("seq1\t3\t9\tname\t0\t-\r\n", bed=True) == (b"seq1", 3, 9, -1)
    assert p("seq1\t3\t9\tname\t0\t+\textra\tmore\n", bed=True) == (b"seq1", 3, 9, 1)
    assert p("seq1\t3\t9\tname\t0\t.\n", bed=True) == (b"seq1", 3, 9, 1)
    assert p("a:b\t3\t9\tname\t0\n", bed=True) == (b"a:b", 3, 9, 1)                                       # five columns: no strand
    for bad in ["seq1\t3\n", "seq1\t3\t\n", "seq1\t9\t3\n", "seq1\t3\t3\n", "seq1\t-1\t3\n", "seq1\t3\t9x\n", "\t3\t9\n", "seq1 3 9\n", "seq1\t3\t9\tn\t0\t?\n",
                "seq1\t3\t9\tn\t0\t+-\n", "seq1\t3\t9\tn\t0\t\n", "seq1\t3\t99999999999999999999\n", ""]:
        assert p(bad, bed=True) is None, bad


def test_library_and_usage():
    from ropebwt3_amd import gpu
    assert "rb3gpu_fetch" in gpu.SYMBOLS
    lib = ctypes.CDLL(_build.LIB_GPU)
    assert hasattr(lib, "rb3gpu_fetch")
    assert ctypes.sizeof(gpu.FetchStats) == 4 * 8 + 7 * 8
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"    fetch " in r.stdout
    r = subprocess.run([CLI, "fetch"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith(b"Usage: ropebwt3-amd fetch") and b"--row" in r.stderr
