"""`remove` on the GPU: the command against the committed indexes and the reference's recorded answers for the sequences that stay
(tests/golden/REMOVE_MANIFEST.json), on both marking paths; its output formats and input formats; the API on random indexes against the oracle's BWT of
the strings that stay -- bitmap word and group borders, the chunked builder on small inputs, the spacings of the pieces, what follows a removal --; the
refusals; the sorted string orders against the live reference."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, host
from ropebwt3_amd.gpu import Rb3GpuError, nt6_of
from tests import remove_model as rm
from tests import util

CLI = _build.BIN_CLI
GOLDEN = util.GOLDEN
MANIFEST = json.load(open(os.path.join(GOLDEN, "REMOVE_MANIFEST.json")))
INDEXES = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
G = lambda x: os.path.join(GOLDEN, x)    # noqa: E731


def _cli(args, timeout=300, env=None, cmd="remove"):
    return subprocess.run([CLI, cmd] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


def _md5(b):
    return hashlib.md5(b).hexdigest()


def _both_strands(idx):
    e = INDEXES[os.path.splitext(idx)[0]]
    return "-R" not in e["flags"] and "-F" not in e["flags"]


def _args(e, tmp_path):
    """the arguments of a recorded case: ranges of rows -- of sequences with --pair where the index holds both strands and the rows are whole pairs --, in a
    file behind -f where there are many"""
    pair = _both_strands(e["index"]) and all(a % 2 == 0 and b % 2 == 1 for a, b in e["rows"])
    rs = [(a // 2, b // 2) if pair else (a, b) for a, b in e["rows"]]
    words = ["%d" % a if a == b else "%d-%d" % (a, b) for a, b in rs]
    out = ["--pair"] if pair else []
    if len(words) > 64:
        fn = tmp_path / "rows.txt"
        fn.write_text("".join(w + "\n" for w in words[1:]))
        return out + ["-f", str(fn), G(e["index"]), words[0]]
    return out + [G(e["index"])] + words


# ---- 1. the committed oracle ----

@pytest.mark.gpu
def test_genomes12_halves_and_the_round_trip(tmp_path):
    first6 = open(G("genomes12_first6.fmd"), "rb").read()
    assert _ok(_cli(["-d", G("genomes12.fmd"), "12-23"])) == first6
    assert _ok(_cli(["-d", "--pieces", G("genomes12.fmd"), "12-23"])) == first6
    e = MANIFEST["genomes12/first6"]
    assert e["rows"] == [[0, 11]]
    for extra in ([], ["--pieces"]):
        out = _ok(_cli(["-d"] + extra + [G("genomes12.fmd"), "0-11"]))
        assert len(out) == e["bytes"] and _md5(out) == e["md5"]
    # remove the last six, add them again: the index the reference built from all twelve
    part = tmp_path / "part.fmd"
    _ok(_cli(["-d", "-o", str(part), "--pair", G("genomes12.fmd"), "6-11"]))
    assert part.read_bytes() == first6
    back = _ok(_cli(["-d", "-i", str(part), G("genomes12_rest6.fa.gz")], cmd="build"))
    assert _md5(back) == INDEXES["genomes12"]["fmd_md5"] and back == open(G("genomes12.fmd"), "rb").read()


# ---- 2. the recorded matrix ----

@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_cli_matches_recorded(key, tmp_path):
    e = MANIFEST[key]
    args = _args(e, tmp_path)
    for extra in ([], ["--pieces"]):
        out = _ok(_cli(["-d"] + extra + args))
        assert len(out) == e["bytes"] and _md5(out) == e["md5"], (key, extra)


# ---- 3. formats ----

@pytest.mark.gpu
def test_output_and_input_formats(tmp_path):
    e = MANIFEST["edge_dups/every_second"]
    args = _args(e, tmp_path)
    want = _ok(_cli(["-d"] + args))
    assert _md5(want) == e["md5"]
    for flags in ([], ["-b"], ["-e"], ["-e", "--bre-run-bytes", "1"]):
        fn = tmp_path / "out.idx"
        _ok(_cli(flags + ["-o", str(fn)] + args))
        raw = fn.read_bytes()
        assert raw[:3] == (b"BRE" if "-e" in flags else b"RB\2"), flags     # FMR unless asked otherwise, as merge
        assert _ok(_cli(["-d", str(fn)], cmd="recode")) == want, flags
    assert _ok(_cli(["-d"] + [a if a != G("edge_dups.fmd") else G("edge_dups.bre") for a in args])) == want
    first6 = MANIFEST["genomes12/middle"]
    assert first6["rows"] == [[10, 11]]
    a = _ok(_cli(["-d", G("genomes12_first6.fmd"), "10-11"]))
    assert _ok(_cli(["-d", G("genomes12_first6.fmr"), "10", "11"])) == a and _ok(_cli(["-d", "--pair", "--pieces", G("genomes12_first6.fmr"), "5"])) == a


@pytest.mark.gpu
def test_verbose_line_has_the_stats():
    r = _cli(["-d", "--pieces", G("edge_dups.fmd"), "0-1"], env=dict(os.environ, RB3_VERBOSE="3", RB3GPU_GET_PIECE="2"))
    assert _md5(_ok(r)) == MANIFEST["edge_dups/first"]["md5"]
    line = [x for x in r.stderr.decode().splitlines() if "[M::main_remove" in x][-1]
    assert "removed 2 strings, " in line and all(w in line for w in ("LF steps", "pieces", "marking ", "rebuild "))


# ---- 4. the API on random indexes ----

def _strings(seed, n, lo=1, hi=200):
    rng = np.random.default_rng(seed)
    g = util.random_genome(rng, 4000)
    out = []
    for i in range(n):
        ln = int(rng.integers(lo, hi + 1))
        s = int(rng.integers(0, g.size - ln))
        t = g[s:s + ln].copy()
        if i % 7 == 3:
            t[ln // 2] = 5                      # an N
        out.append(t)
    out[5] = out[4].copy()                      # duplicates, next to each other and apart
    out[n - 1] = out[0].copy()
    out[9] = np.zeros(0, dtype=np.uint8)        # a string of no symbols
    return out


def _bwt(strs):
    return util.Oracle().bwt(util.make_text(strs, rev=False))


_BASE = {}


def _base():
    """100 strings of 0 .. 200 symbols, their BWT and whose walk stands on the last row: computed once, shared, never changed"""
    if not _BASE:
        strs = _strings(11, 100)
        b = _bwt(strs)
        fm = rm.Fm(b)
        owner = [r for r in range(len(strs)) if rm.mark(fm, [r])[0][fm.n - 1]]
        assert len(owner) == 1
        _BASE.update(strs=strs, b=b, last_owner=owner[0])
    return _BASE


def _check(h, strs, gone, pieces, st=None):
    """remove `gone` from the handle that holds `strs`; the index is then the oracle's BWT of the rest.  Returns the rest"""
    rest = [s for r, s in enumerate(strs) if r not in set(gone)]
    want = _bwt(rest)
    st = {} if st is None else st
    h.remove(gone, pieces=pieces, stats=st)
    assert h.get_tot() == want.size and np.array_equal(h.export_plain(), want), (gone, pieces)
    assert h.get_acc().tolist() == [0] + np.cumsum(np.bincount(want, minlength=6)).tolist()
    d = sorted(set(gone))
    assert st["n_strings"] == len(d) and st["n_rows"] == sum(strs[r].size + 1 for r in d)
    assert st["removed"] == [len(d)] + [sum(int((strs[r] == c).sum()) for r in d) for c in range(1, 6)]
    return rest


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [False, True])
def test_api_rows_words_and_borders(pieces):
    B = _base()
    strs = B["strs"]
    h = Rb3Gpu(verbose=1)
    try:
        cases = [[3], [0, B["last_owner"]], [31, 32, 63, 64], [9], [4, 5], [7, 7, 2, 7, 2], list(range(1, 100)), list(range(0, 100, 2))]
        for gone in cases:          # one strand alone, the first row and the last, the borders of the bitmap's words, the empty string, duplicates twice over
            h.from_plain(B["b"])
            st = {}
            _check(h, strs, gone, pieces, st)
            assert (st["n_pieces"] > 0) == pieces and st["n_steps"] >= st["n_rows"]
        h.from_plain(B["b"])
        h.remove([], pieces=pieces)                                   # n == 0: nothing changes
        assert np.array_equal(h.export_plain(), B["b"])
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("left", [8192, 16384, 8191, 100])
def test_api_length_that_stays(left):
    """what stays is exactly one group of 8192 symbols, exactly two, one symbol less, and a fraction of one"""
    rng = np.random.default_rng(left)
    keep = [util.random_genome(rng, 127) for _ in range(left // 128)]
    if left % 128:
        keep.append(util.random_genome(rng, left % 128 - 1))
    extra = [util.mutate(rng, keep[i % len(keep)], 0.05) for i in range(40)]
    strs = []
    for i, s in enumerate(keep):                                   # the strings that go lie among those that stay
        strs.append(s)
        if i < len(extra):
            strs.append(extra[i])
    strs += extra[len(keep):]
    gone = [r for r, s in enumerate(strs) if any(s is x for x in extra)]
    assert sum(s.size + 1 for r, s in enumerate(strs) if r not in gone) == left
    h = Rb3Gpu(verbose=1)
    try:
        for pieces in (False, True):
            h.from_plain(_bwt(strs))
            _check(h, strs, gone, pieces)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key,val", [("load_chunk", 1), ("load_chunk", 2), ("get_piece", 2), ("get_piece", 4), ("get_piece", 8), ("get_piece", 20)])
def test_api_chunks_and_spacings(key, val):
    """chunks of one and two groups: the builder asks for ranges that start and end inside the old index's groups; spacings from 4 rows to one piece per string"""
    rng = np.random.default_rng(5)
    g = util.random_genome(rng, 3000)
    strs = [util.mutate(rng, g, 0.03) for _ in range(12)] + _base()["strs"][:40]     # ~41 k symbols: six groups
    gone = [1, 4, 5, 13, 30, 51]
    h = Rb3Gpu(verbose=1)
    try:
        h.tune(key, val)
        for pieces in ((False, True) if key == "load_chunk" else (True,)):
            h.from_plain(_bwt(strs))
            st = {}
            _check(h, strs, gone, pieces, st)
            if pieces:
                m, n = len(strs), sum(s.size + 1 for s in strs)
                S = val if key == "get_piece" else 8
                assert st["n_pieces"] == m + -(-(n - m) // (1 << S)) and 0 < st["max_piece_steps"]
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [False, True])
def test_api_what_follows_a_removal(pieces):
    B = _base()
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(B["b"])
        h.keep_ssa(3)
        assert h.ssa_info() is not None
        rest = _check(h, B["strs"], [2, 50, 98], pieces)
        assert h.ssa_info() is None                                  # the sampled suffix array belonged to the old index
        rest = _check(h, rest, [0, 1, 96], pieces)                   # a second removal: the strings are numbered as they now stand
        end, seqs = h.retrieve(range(len(rest)), pieces=pieces)
        assert (end >= 0).all() and len(seqs) == len(rest) and all(np.array_equal(a, b) for a, b in zip(seqs, rest))
        more = [s for s in _strings(12, 10) if s.size]
        h.merge_plain(_bwt(more))                                    # a further batch merges into what is left
        assert np.array_equal(h.export_plain(), _bwt(rest + more))
        h.keep_ssa(3)
        assert h.ssa_info() is not None
    finally:
        h.close()


# ---- 5. refusals ----

@pytest.mark.gpu
def test_cli_refusals(tmp_path):
    idx = G("edge_dups.fmd")       # 12 strings, 6 sequences
    bad = tmp_path / "rows.txt"
    bad.write_text("1\n2x\n")
    for args in ([idx, "abc"], [idx, "3", "2-"], [idx, "5-3"], [idx, "12"], [idx, "0-12"], ["--pair", idx, "6"], [idx], [idx, "0-11"], ["--pair", idx, "0-5"], ["--pieces", idx, "0-11"],
                 ["-f", str(bad), idx], ["--pair", G("k2_fwd.fmd"), "0"], [idx, "-1"]):
        out = tmp_path / "never.fmd"
        r = _cli(["-d", "-o", str(out)] + args)
        err = r.stderr.decode().strip().splitlines()
        assert r.returncode == 1 and r.stdout == b"" and not out.exists(), args
        assert len(err) == 1 and err[0].startswith(("ERROR", "remove: ")), (args, err)


@pytest.mark.gpu
def test_api_refusals_leave_the_index():
    B = _base()
    h, empty = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        h.from_plain(B["b"])
        m = len(B["strs"])
        for pieces in (False, True):
            for rows in ([m], [-1], [0, m + 5], list(range(m)), list(range(m)) + [3]):
                with pytest.raises(Rb3GpuError) as e:
                    h.remove(rows, pieces=pieces)
                assert e.value.code == -3
                assert h.get_acc()[1] == m and np.array_equal(h.export_plain(), B["b"])
            with pytest.raises(Rb3GpuError) as e:
                empty.remove([0], pieces=pieces)
            assert e.value.code == -5
    finally:
        h.close()
        empty.close()


# ---- 6. the sorted string orders, against the live reference ----

@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["-r", "-s"])
def test_ordered_indexes_against_the_live_reference(flag, tmp_path):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    import gzip
    lines = gzip.open(G("reads_fq.fa.gz")).read().decode().split("\n")
    step = 4 if lines[0].startswith("@") else 2                     # FASTQ or FASTA, one line per sequence
    recs = [(">" + lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, step) if lines[i][:1] in (">", "@")]
    assert len(recs) == 3052
    full, rest = tmp_path / "full.fa", tmp_path / "rest.fa"
    full.write_text("".join("%s\n%s\n" % r for r in recs))
    idx = tmp_path / "full.fmr"
    idx.write_bytes(_ok(subprocess.run([util.REF_BIN, "build", "-t4", "-b", flag, str(full)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)))
    # in a sorted order the strings of a sequence are where their order puts them: which rows hold the 100 sequences is asked of the index itself
    text = _ok(_cli(["--all", str(idx)], cmd="get")).decode().split("\n")
    seqs = [nt6_of(x) for x in text[1::2]]
    assert len(seqs) == 6104
    gone_recs = set(range(7, 3052, 30)[:100])
    gone_strs = {}
    for i in gone_recs:
        s = nt6_of(recs[i][1])
        for t in (s, util.revcomp(s)):
            gone_strs[t.tobytes()] = gone_strs.get(t.tobytes(), 0) + 1
    rows = []
    for r, s in enumerate(seqs):
        k = s.tobytes()
        if gone_strs.get(k, 0) > 0:
            gone_strs[k] -= 1
            rows.append(r)
    assert len(rows) == 200
    rest.write_text("".join("%s\n%s\n" % r for i, r in enumerate(recs) if i not in gone_recs))
    want = _ok(subprocess.run([util.REF_BIN, "build", "-t4", "-d", flag, str(rest)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300))
    rf = tmp_path / "rows.txt"
    rf.write_text("".join("%d\n" % r for r in rows))
    for extra in ([], ["--pieces"]):
        assert _ok(_cli(["-d"] + extra + ["-f", str(rf), str(idx)])) == want, (flag, extra)
    r = _cli(["-d", "--pair", str(idx), "7"])          # rows 2i and 2i + 1 are no sequence here
    assert r.returncode == 1 and r.stdout == b"" and len(r.stderr.decode().strip().splitlines()) == 1 and b"--pair" in r.stderr
    out = _ok(_cli(["-f", str(rf), str(idx)]))         # the FMR output keeps the order byte of its input
    assert out[:4] == idx.read_bytes()[:4] and out[3] in (1, 2)
