"""The GPU FMD packer (rb3gpu_fmdenc.hip: k_fe_width, k_fe_table, k_fe_chain1, k_fe_emit, k_fe_special, k_fe_pack, driven by
rb3fmd_enc_piece) and decoder (k_fd_count, k_fd_fill, k_fd_fill_range, k_fd_long) on run lists crafted to sit on the borders of
the algorithm (tests/fmd_cases.py), straight through the API -- no text, no CLI, and no host fallback: export_fmd_words raises the
packer's own error.  The expected words are always those of tests/fmd_model.py, which test_cpu_fmd.py pins to the reference; every
case first asserts through the model's chain that it sits on its border, every comparison is exact, and every failure names the
block (fmd_model.describe)."""
import hashlib
import json
import os
import subprocess
import time

import numpy as np
import pytest

from ropebwt3_amd import _build
from ropebwt3_amd.gpu import Rb3Gpu, Rb3GpuError
from tests import fmd_cases as C
from tests import fmd_model as M
from tests import util

pytestmark = pytest.mark.gpu

EDGE = json.load(open(os.path.join(util.GOLDEN, "FMDEDGE_MANIFEST.json")))
CLI = _build.BIN_CLI
ESYMBOL, EUNSUP = -4, -7
PIECES = (0, 32768, 50000)      # rb3gpu_tune "fmd_piece": the default (64 M runs), the least the driver takes, a size that is no whole group
ONE_PASS = 1 << 20              # a load_chunk no stream here exceeds

_model = {}                     # case -> (lens, syms, chain, words): computed once, never changed; of the 10^8-run cases only P7a, which two tests use


def model_of(name):
    if name not in _model:
        if name.startswith("P7"):
            plain = C.super_plain(name[2])
            lens, syms = M.runs_of_plain(plain)
            ch = M.chain(lens)
            C.check_super(name[2], ch)
        else:
            lens, syms = C.small(name)
            ch = M.chain(lens)
            C.check_small(name, lens, ch)
        words = M.pack(lens, syms, ch)
        for a in (lens, syms, words):
            a.setflags(write=False)
        if name.startswith("P7") and name != "P7a":
            return lens, syms, ch, words
        _model[name] = (lens, syms, ch, words)
    return _model[name]


def equal(got, want, ch, what):
    assert got.size == want.size and np.array_equal(got, want), "%s: %s" % (what, M.describe(got, want, ch))


# (Rb3Gpu.from_runs and from_fmd_file take a list of tuples and a file; the cases here are numpy arrays of up to 120000 runs and word
# streams that exist only in memory, so the two C entry points are called on the arrays directly)
def from_runs(h, lens, syms):
    arr = (lens.astype(np.uint64) << np.uint64(3)) | syms.astype(np.uint64)
    h._chk(h._lib.rb3gpu_from_runs(h._h, arr.size, arr.ctypes.data), "rb3gpu_from_runs")


def from_words(h, words, mcnt):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    mc = None if mcnt is None else np.ascontiguousarray(mcnt, dtype=np.int64)
    h._chk(h._lib.rb3gpu_from_fmd_words(h._h, words.size, words.ctypes.data, None if mc is None else mc.ctypes.data), "rb3gpu_from_fmd_words")


def check_counts_and_ranks(h, lens, syms):
    """get_acc and rank1a at both ends of every run against the cumulative counts of the run list"""
    cnt = C.sym_counts(lens, syms)
    assert np.array_equal(h.get_acc(), np.concatenate([[0], np.cumsum(cnt)]))
    k = np.concatenate([[0], np.cumsum(lens)])
    cm = np.zeros((lens.size + 1, 6), dtype=np.int64)
    for c in range(6):
        np.cumsum(np.where(syms == c, lens, 0), out=cm[1:, c])
    got = h.rank1a(k)
    bad = np.flatnonzero((got != cm).any(axis=1))
    assert bad.size == 0, "rank1a differs at %d run borders, first at position %d: %s != %s" % (bad.size, k[bad[0]], got[bad[0]].tolist(), cm[bad[0]].tolist())


# ---- the packer ----

@pytest.mark.parametrize("name", C.SMALL)
def test_packer_on_its_borders(name):
    """P1 blocks of 95 codes and the largest chunk entry offset; P2 a block before of 0x3fff / 0x4000 symbols; P3 both header types
    interleaved, in two pieces; P4 every code width class; P5 a final piece of a handful of runs, a chunk of them, a whole group"""
    lens, syms, ch, want = model_of(name)
    h = Rb3Gpu(verbose=1)
    try:
        from_runs(h, lens, syms)
        for piece in PIECES:
            h.tune("fmd_piece", piece)
            equal(h.export_fmd_words(), want, ch, "%s, fmd_piece %d" % (name, piece))
    finally:
        h.close()


@pytest.mark.parametrize("case", ["a", "d", "e", "b", "c"])
def test_packer_at_the_superblock_border(case):
    """P7: 10^8 runs of one symbol each, the smallest index in which a superblock of 2^20 blocks ends.  a: the short block 2^20 - 1
    holds 79 codes and block 2^20 counts them; d: it carries a 32-bit header and 192 payload bits; b: the data end inside it and the
    trailing header opens superblock 1; c: the trailing header IS block 2^20 - 1.  Packed in two pieces (the default), in pieces of
    32768, 50000 and -- a, d, e -- 3 000 000 runs (the border inside a piece whose block numbers are its own) and -- a, e -- in pieces
    of 3040 groups.  No piece size makes a piece of run list a BEGIN with block 2^20 - 1 (pieces end on multiples of 8192 runs; the
    driver restated in fmd_cases.piece_split shows the block at hand falling 1 to 43 blocks short for every size): there the fourth
    piece begins with block 2^20 - 2.  e is a with its first 16 runs two symbols long, which moves the block starts so that the fourth
    piece does begin with block 2^20 - 1: k_fe_special then runs on block 1 of a piece, whose block before is the carried one, and
    the emit list is cut behind its first entry.  These cases do not exist smaller; most of a case's time is the model on the host.
    Measured on an MI355X, seconds per case a / d / e / b / c: the whole test 9.1 / 9.2 / 9.0 / 8.3 / 8.2, of which the model (chain,
    pack, md5) 5.5 / 5.5 / 5.3 / 4.9 / 4.8 and from_plain 0.38 / 0.55 / 0.54 / 0.35 / 0.36; export_fmd_words in two pieces (the
    default) 0.03, in pieces of 3040 groups 0.04, of 3 000 000 runs 0.06, of 50000 runs 1.2, of 32768 runs 1.7 (3040 pieces);
    `plain2fmd` of the host CLI on the same 10^8 symbols 1.1 s on one CPU core."""
    t0 = time.perf_counter()
    lens, syms, ch, want = model_of("P7" + case)
    ent = EDGE[case]
    assert want.size == ent["n_words"] and hashlib.md5(want.tobytes()).hexdigest() == ent["data_md5"], "the model differs from what the reference wrote"
    t1 = time.perf_counter()
    settings = list(PIECES) + ([3000000] if case in "ade" else [])
    if case == "a":
        assert C.SB - 2 in C.piece_split(ch.first_run, lens.size, C.PIECE_FIRST)[0]
    if case in "ae":
        settings.append(C.PIECE_FIRST)
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(C.super_plain(case))
        t2 = time.perf_counter()
        times = []
        for piece in settings:
            h.tune("fmd_piece", piece)
            t = time.perf_counter()
            got = h.export_fmd_words()
            times.append("%d: %.2f" % (piece, time.perf_counter() - t))
            equal(got, want, ch, "P7%s, fmd_piece %d" % (case, piece))
        print("P7%s: model %.1f s, from_plain %.2f s, export_fmd_words by fmd_piece %s s" % (case, t1 - t0, t2 - t1, ", ".join(times)))
    finally:
        h.close()


@pytest.mark.parametrize("which", ["a", "b"])
def test_header_width_at_two_to_the_thirty(which, tmp_path):
    """P6 / D3: a block before of exactly 2^30 - 1 (a) or 2^30 (b) symbols, written by the host writer and loaded chunk by chunk (never
    one byte per symbol).  Both decode to their runs, counts and ranks -- b through a type-2 block: 7 header words, one payload word.
    a is packed on the GPU with a 32-bit header behind the large block; b is the packer's hand-over: EUNSUP under every piece setting,
    and `build -d -i` writes the file through the host encoder"""
    lens, syms = C.wide(which)
    ch = M.chain(lens)
    C.check_wide(which, lens, ch)
    want = M.pack(lens, syms, ch)
    l2, s2 = M.unpack(want)
    assert np.array_equal(l2, lens) and np.array_equal(s2, syms), "every block decodes on its own: no run straddles two"
    fn = C.host_fmd_file(lens, syms, tmp_path / (which + ".fmd"))
    raw = open(fn, "rb").read()
    equal(C.fmd_data_words(raw)[0], want, ch, "the host writer")
    if which == "b":
        assert M.header_counts(want, 1) == (2, [1 << 30] + C.sym_counts(lens[:13], syms[:13]).tolist()) and ch.n_runs[1] == 1
    h = Rb3Gpu(verbose=1)
    try:
        h.from_fmd_file(fn)
        assert h.get_tot() == int(lens.sum())
        assert h.export_runs() == list(zip(syms.tolist(), lens.tolist()))
        check_counts_and_ranks(h, lens, syms)
        for piece in PIECES:
            h.tune("fmd_piece", piece)
            if which == "a":
                got = h.export_fmd_words()
                equal(got, want, ch, "P6a, fmd_piece %d" % piece)
                assert M.header_counts(got, 1)[0] == 1
            else:
                with pytest.raises(Rb3GpuError) as e:
                    h.export_fmd_words()
                assert e.value.code == EUNSUP
    finally:
        h.close()
    if which == "b":
        r = subprocess.run([CLI, "build", "-d", "-i", fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-600:]
        assert r.stdout == raw
        assert b"packed the FMD on the GPU" not in r.stderr


# ---- the decoder ----

def load_and_check(words, lens, syms, want, chunk, what, runs=True):
    """want: the symbols of the runs, one byte each"""
    h = Rb3Gpu(verbose=1)
    try:
        h.tune("load_chunk", chunk)
        from_words(h, words, C.sym_counts(lens, syms))
        assert h.get_tot() == int(lens.sum()), what
        got = h.export_plain()
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            j = int(np.searchsorted(np.cumsum(lens), i, side="right"))
            raise AssertionError("%s: the symbols differ first at position %d, in run %d (%d symbols of %d): %d" % (what, i, j, lens[j], syms[j], got[i]))
        if runs:
            assert h.export_runs() == list(zip(syms.tolist(), lens.tolist())), what
        assert np.array_equal(h.get_acc(), np.concatenate([[0], np.cumsum(C.sym_counts(lens, syms))])), what
    finally:
        h.close()


@pytest.mark.parametrize("name", C.SMALL + ["P7a"])
def test_decoder_round_trip(name):
    """D1: the model's words of the packer cases through rb3gpu_from_fmd_words, in one pass and in chunks of 1 and 3 groups; P7a has
    the header block behind a superblock border and the short block in front of it"""
    lens, syms, ch, words = model_of(name)
    want = M.expand(lens, syms)
    for chunk in (ONE_PASS, 1, 3):
        load_and_check(words, lens, syms, want, chunk, "%s, load_chunk %d" % (name, chunk), runs=lens.size <= 120000)


def test_decoder_long_runs_at_chunk_borders():
    """D2: runs of 65535, 65536, 70000 and 200000 symbols, each once beginning 5 symbols before a chunk border and once ending 3 behind
    one (one run cannot do both: none of the lengths is 8 modulo 8192), destinations of every residue modulo 8.  Chunks of one group
    clip every part below FD_LONG (k_fd_fill_range's own loops); chunks of nine groups leave parts on both sides of it (k_fd_long)"""
    lens, syms, marks = C.long_runs()
    C.check_long_runs(lens, marks)
    words, want = M.pack(lens, syms), M.expand(lens, syms)
    for chunk in (1, 9, ONE_PASS):
        load_and_check(words, lens, syms, want, chunk, "load_chunk %d" % chunk)


def test_decoder_refusals():
    """D4: a symbol field of 6 and of 7, a stream of zeros, counts in the file header that are off by one with and without the total
    changing: each is ESYMBOL, on the one-pass and on the chunked path, and the handle then loads the good stream"""
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 41, size=3000).astype(np.int64)
    syms = C.alt(lens.size)
    ch = M.chain(lens)
    good = M.pack(lens, syms, ch)
    mc = C.sym_counts(lens, syms)
    assert int(lens.sum()) > 3 * 8192 and ch.first_run.size > 40
    bad = []
    for v, blk in ((6, 0), (7, 17)):
        w = good.copy()
        sh = np.uint64(64 - int(M.widths(lens[ch.first_run[blk]:ch.first_run[blk] + 1])[0]))   # the symbol of the block's first code
        w[8 * blk + 2] = (w[8 * blk + 2] & ~(np.uint64(7) << sh)) | np.uint64(v) << sh
        assert ch.type[blk] == 0
        with pytest.raises(ValueError):
            M.unpack(w)
        bad.append(("symbol %d" % v, w, mc))
    bad.append(("zeros", np.zeros(64, dtype=np.uint64), None))
    m2, m3 = mc.copy(), mc.copy()
    m2[1] += 1; m2[2] -= 1
    m3[1] += 1
    bad += [("counts off by one, same total", good, m2), ("counts off by one", good, m3)]
    for chunk in (ONE_PASS, 1):
        h = Rb3Gpu(verbose=1)
        try:
            h.tune("load_chunk", chunk)
            for what, w, m in bad:
                with pytest.raises(Rb3GpuError) as e:
                    from_words(h, w, m)
                assert e.value.code == ESYMBOL, (what, chunk)
                from_words(h, good, mc)
                check_counts_and_ranks(h, lens, syms)
        finally:
            h.close()
