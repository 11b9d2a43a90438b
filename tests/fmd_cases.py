"""The run lists test_cpu_fmd.py and test_gpu_fmd.py put on the borders of the FMD packer and decoder, each with the condition --
stated through fmd_model.chain -- that it really sits there.  Test infrastructure only."""
import functools

import numpy as np

from tests import fmd_model as M

SB = M.SB_BLOCKS
FE_CHUNK = 4096                      # runs per speculation chunk of the packer (rb3gpu_fmdenc.hip)
SB0_RUNS = (SB - 1) * 95 + 79        # runs of length 1 in superblock 0: 95 codes of 4 bits in 384 bits, 79 in the short last block


def alt(n, k=6):
    """n symbols 0..k-1 in turn: neighbours differ"""
    return (np.arange(n, dtype=np.int64) % k).astype(np.uint8)


def chunk_entries(ch, n_runs):
    """per chunk of FE_CHUNK runs: (offset of the first block start in it, that block's type)"""
    k = np.arange(0, (n_runs + FE_CHUNK - 1) // FE_CHUNK, dtype=np.int64)
    b = np.searchsorted(ch.first_run, k * FE_CHUNK, side="left")
    return ch.first_run[b] - k * FE_CHUNK, ch.type[b]


def piece_split(first_run, n, piece, m=0):
    """The driver of the packer (rb3gpu_export_fmd_words) restated for a BWT of n runs of which the first m hold two symbols and all
    others one (2 m <= 8192): every group of 8192 symbols then holds 8192 runs, the first m fewer.  At most `piece` runs (32768 at
    least) make one piece; otherwise the packer gets whole groups, as many as leave a group's worth of room behind what it carried
    over; a piece that is not the last stops at the first block that begins in its last whole chunk 128 runs before its end and
    carries the runs from the block before that one on.  first_run: the model's block starts (None: only the split is wanted).
    Returns (the global numbers of the blocks the pieces after the first begin with, the new runs the final piece gets)."""
    G = 8192
    piece = max(piece, 32768) if piece > 0 else 64 << 20      # (0: the default)
    if n <= piece:
        return [], n
    ngrp, cap = (n + m + G - 1) // G, piece + 2 * G + 1024

    def before(g):
        return 0 if g == 0 else min(g * G - m, n)
    ga, nc, base, hands = 0, 0, 0, []
    while True:
        room = min(cap - nc, piece + G)
        gb = min(ngrp, ga + (room - G) // G + 1)
        while gb > ga + 1 and before(gb) - before(ga) > room - G:
            gb -= 1
        if gb == ngrp:
            return hands, before(gb) - before(ga)
        nloc = nc + before(gb) - before(ga)
        if first_run is not None:
            b = int(np.searchsorted(first_run, base + (nloc - 1 - 128) // FE_CHUNK * FE_CHUNK, side="left"))
            hands.append(b)
            cs = int(first_run[b - 1])
            nc, base = base + nloc - cs, cs
        ga = gb


# ---- the small cases: name -> (lens, syms); check_small(name, lens, chain) asserts the border ----

def _p1():
    return np.ones(120000, dtype=np.int64)


def _p2(which):
    head = [819] * 19 + [822] if which == "a" else [819] * 16 + [820] * 4
    return np.array(head + [700] * 60, dtype=np.int64)


def _p3():
    rng = np.random.default_rng(20260)
    return rng.choice(np.array([1, 1, 1, 2, 7, 300, 16383, 16384, 40000], dtype=np.int64), size=40000, p=[0.3, 0.3, 0.3, 0.04, 0.025, 0.02, 0.005, 0.005, 0.005])


def _p4():
    out = []
    for k in list(range(1, 27)) + [16]:
        out += [(1 << k) - 1, 1 + k % 3, 1 << k, 1, 2 + k % 2]
    return np.array(out, dtype=np.int64)


# P5: runs of length 1; the new runs the final piece gets at fmd_piece 32768 (pieces of four groups of 8192 runs).  Only there is the last
# piece small: at 50000 it has 16384 new runs or more, and by default everything is one piece.  65536 + 4095 is not in the issue's list;
# it is the count whose last piece really is about a chunk.
P5_LAST = {65536: 32768, 65537: 1, 65536 + 4095: 4095, 73728: 8192, 73729: 8193, 73728 + 4095: 12287}
P5_RUNS = tuple(P5_LAST)


@functools.lru_cache(maxsize=None)
def small(name):
    if name == "P1":
        lens = _p1()
    elif name in ("P2a", "P2b"):
        lens = _p2(name[2])
    elif name == "P3":
        lens = _p3()
    elif name == "P4":
        lens = _p4()
    elif name.startswith("P5_"):
        lens = np.ones(int(name[3:]), dtype=np.int64)
    else:
        raise KeyError(name)
    lens.setflags(write=False)
    syms = alt(lens.size)
    syms.setflags(write=False)
    return lens, syms


SMALL = ["P1", "P2a", "P2b", "P3", "P4"] + ["P5_%d" % r for r in P5_RUNS]


def check_small(name, lens, ch):
    nb = ch.first_run.size - 1
    if name == "P1":
        assert (ch.n_runs[:nb - 1] == 95).all() and (ch.type == 0).all()
        off, _ = chunk_entries(ch, lens.size)
        assert off[26] == 94 and off.max() == 94, "chunk 26 (runs 106496..) is entered at the largest offset a type-0 chain has"
    elif name in ("P2a", "P2b"):
        a = name == "P2a"
        assert ch.n_runs[0] == 20 and ch.n_sym[0] == (0x3fff if a else 0x4000)
        assert ch.type[1] == (0 if a else 1) and ch.n_runs[1] == (20 if a else 13)
    elif name == "P3":
        assert int(lens.sum()) < (64 << 20)
        assert {0, 1} == set(ch.type.tolist())
        _, ty = chunk_entries(ch, lens.size)
        assert {0, 1} == set(ty[1:].tolist()), "some chunk is entered in each header type"
        assert lens.size > 32768, "two pieces at fmd_piece 32768"
    elif name == "P4":
        y = M.ilog2(lens)
        assert {0, 1, 2, 3, 4} == set(M.ilog2(y + 1).tolist()), "every class of y + 1 up to 2^26"
        # (the issue's list, k = 1 .. 26, sums to 268 M symbols: its own "below 200 M" cannot hold, so the bound here is 2^29)
        assert int(lens.sum()) < (1 << 29) and int(M.widths(lens).max()) == 2 * 4 + 1 + 26 + 3
    else:
        n = int(name[3:])
        assert (lens == 1).all() and lens.size == n
        assert piece_split(None, n, 32768)[1] == P5_LAST[n] and piece_split(None, n, 50000)[1] >= 16384 and piece_split(None, n, 0)[1] == n
        assert {1, 4095, 8192} <= set(P5_LAST.values()), "a last piece of one run, of a chunk less one, of a whole group"


# ---- header width at 2^30: streams of about 40 runs ----

@functools.lru_cache(maxsize=None)
def wide(which):
    """(lens, syms): block 0 holds exactly 2^30 - 1 ("a") or 2^30 ("b") symbols"""
    head = [1 << k for k in range(29, 21, -1)] + [(1 << 22) - (5 if which == "a" else 4), 1, 1, 1, 1]   # 2^30 - 2^22, then the rest
    tail = [1 << 24, 70000, 1, 2, 1 << 20, 5, 16383, 16384, 3, 1 << 26, 1, 1, 40000, 9, 1 << 28, 2, 65536, 1, 7, 300, 1 << 21, 1, 4, 123456, 1, 1, 1 << 25]
    lens = np.array(head + tail, dtype=np.int64)
    return lens, alt(lens.size)


def check_wide(which, lens, ch):
    assert ch.n_runs[0] == 13 and ch.n_sym[0] == (1 << 30) - (1 if which == "a" else 0)
    assert ch.type[1] == (1 if which == "a" else 2), "the header behind the large block"
    assert int(lens.sum()) < (1 << 32) and int(lens.sum()) > (16384 << 13), "below 2^32 symbols, above one chunk of the default load_chunk"
    if which == "b":
        assert M.HDR_WORDS[2] == 7 and M.payload_bits(1, 2) == 64 and ch.n_runs[1] >= 1


# ---- the superblock: runs of length 1 (one byte of plain text per run), block 2^20 - 1 is the short one ----

SUPER = {"a": SB0_RUNS + 5000, "b": (SB - 1) * 95 + 40, "c": (SB - 1) * 95, "d": SB0_RUNS + 5000, "e": 99619692}
E_LONG = 16                          # case e: as a, but the first 16 runs hold two symbols, which moves every block start against the
PIECE_FIRST = 3040 * 8192            # grid of chunks and groups so that in pieces of 3040 groups the fourth BEGINS with block 2^20 - 1


def super_lens(case):
    lens = np.ones(SUPER[case], dtype=np.int64)
    if case == "d":
        lens[(SB - 2) * 95] = 20000
    if case == "e":
        lens[:E_LONG] = 2
    return lens


def super_plain(case):
    """the plain BWT of the case, one symbol per byte (symbols 1..4 in turn)"""
    n = SUPER[case]
    syms = (alt(n, 4) + 1).astype(np.uint8)
    return M.expand(super_lens(case), syms) if case in "de" else syms


def check_super(case, ch):
    nb = ch.first_run.size - 1     # data blocks; block nb is the trailing header
    if case == "a":
        assert nb > SB and ch.n_runs[SB - 1] == 79 and (ch.n_runs[:SB - 1] == 95).all()
        assert ch.first_run[SB] == SB0_RUNS and ch.n_sym[SB - 1] == 79, "the header of block 2^20 counts 79"
    elif case == "e":
        assert nb > SB and ch.n_runs[SB - 1] == 79 and ch.n_runs[SB - 2] == 95 and ch.first_run[SB] + 5000 == SUPER["e"]
        hands, _ = piece_split(ch.first_run, SUPER["e"], PIECE_FIRST, E_LONG)
        assert SB - 1 in hands, "block 2^20 - 1 is the block a piece begins with: it starts in the piece's first 128 runs"
        assert 2 * E_LONG <= 8192
    elif case == "b":
        assert nb == SB and ch.n_runs[SB - 1] == 40, "the data end inside the short block; the trailing header opens superblock 1"
    elif case == "c":
        assert nb == SB - 1 and ch.n_runs[SB - 2] == 95, "the trailing header is block 2^20 - 1"
    else:
        assert nb > SB and ch.first_run[SB - 2] == (SB - 2) * 95 and ch.n_sym[SB - 2] >= 0x4000
        assert ch.type[SB - 1] == 1 and M.payload_bits(SB - 1, 1) == 192 and ch.n_runs[SB - 1] == 47, "a 32-bit header and 192 payload bits: 47 codes of 4 bits"
        assert ch.type[SB] == 0


def super_n_words(case, ch):
    nb = ch.first_run.size - 1
    return 8 * nb + M.HDR_WORDS[int(ch.type[nb])]


# ---- long runs at the borders of decode chunks ----

FD_LONG = 65536


@functools.lru_cache(maxsize=None)
def long_runs():
    """(lens, syms): runs of 65535, 65536, 70000 and 200000 symbols, each once beginning 5 symbols before a multiple of 8192 and once
    ending 3 symbols behind one, with runs of 17..24 symbols between them"""
    lens, pos, fill = [], 0, 0

    def pad_to(target):
        nonlocal pos, fill
        assert target >= pos
        while target - pos > 64:
            lens.append(17 + fill % 8)
            pos += lens[-1]
            fill += 1
        if target > pos:
            lens.append(target - pos)
            pos = target
    marks = []
    for L in (65535, 65536, 70000, 200000):
        pad_to(((pos + 200) // 8192 + 1) * 8192 - 5)
        marks.append((pos, L)), lens.append(L)
        pos += L
        m = (pos + 200 + L) // 8192 + 1
        pad_to(8192 * m + 3 - L)
        marks.append((pos, L)), lens.append(L)
        pos += L
    pad_to(pos + 1000)
    lens = np.array(lens, dtype=np.int64)
    return lens, alt(lens.size), marks


def clipped_parts(lens, chunk_sym):
    """lengths of the parts the runs of 65535 symbols and more are cut into by chunks of chunk_sym symbols"""
    S = np.concatenate([[0], np.cumsum(lens)])
    out = []
    for j in np.flatnonzero(lens >= 65535):
        a, e = int(S[j]), int(S[j + 1])
        while a < e:
            nx = min(e, (a // chunk_sym + 1) * chunk_sym)
            out.append(nx - a)
            a = nx
    return out


def check_long_runs(lens, marks):
    S = np.concatenate([[0], np.cumsum(lens)])
    assert int(S[-1]) < 1000000
    for i, (p, L) in enumerate(marks):
        assert (p % 8192 == 8192 - 5) if i % 2 == 0 else ((p + L) % 8192 == 3), (p, L)
    big = lens >= 16
    assert set((S[:-1][big] % 8).tolist()) == set(range(8)) and set((S[1:][big] % 8).tolist()) == set(range(8)), "every residue of the head and tail loops"
    assert max(clipped_parts(lens, 8192)) < FD_LONG, "chunks of one group cut every run below FD_LONG"
    parts = clipped_parts(lens, 9 * 8192)
    assert max(parts) >= FD_LONG and min(parts) < FD_LONG, "chunks of nine groups leave parts on both sides of FD_LONG"


# ---- the host writer (rb3h_fmdw_*) and the pieces of an .fmd file ----

def host_fmd_file(lens, syms, path):
    """the .fmd of the runs, written by the host writer: rb3h_fmdw_enc / _finish / _dump_file"""
    import ctypes
    from ropebwt3_amd import host
    H = host.load_library()
    H.rb3h_fmdw_dump_file.restype = ctypes.c_int
    H.rb3h_fmdw_dump_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    w = H.rb3h_fmdw_init()
    try:
        for l, c in zip(np.asarray(lens).tolist(), np.asarray(syms).tolist()):
            assert H.rb3h_fmdw_enc(w, l, c) == 0
        assert H.rb3h_fmdw_finish(w) == 0
        assert H.rb3h_fmdw_dump_file(w, str(path).encode()) == 0
    finally:
        H.rb3h_fmdw_destroy(w)
    return str(path)


def fmd_data_words(raw):
    """(the data section of an .fmd file as uint64 words, the file header's symbol counts)"""
    raw = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else raw
    assert raw[:4].tobytes() == b"RLD\x03"
    n_bytes = int(raw[16:24].view(np.uint64)[0])
    return raw[80:80 + n_bytes].view(np.uint64), raw[32:80].view(np.uint64).astype(np.int64)


def sym_counts(lens, syms):
    """symbols of each kind 0..5"""
    lens, syms = np.asarray(lens, dtype=np.int64), np.asarray(syms)
    return np.array([int(lens[syms == c].sum()) for c in range(6)], dtype=np.int64)
