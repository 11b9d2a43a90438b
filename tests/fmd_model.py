"""The data section of an .fmd file restated in plain Python/numpy: no GPU, no project library.

Test infrastructure only.  The format (rld0.c:45-51, 107-151, 206-216; rld0.h):

* a run of length l and symbol c is the code delta(l) << 3 | c, where delta is the Elias-delta code of l: with y = ilog2(l) and
  z = ilog2(y + 1) it is z zeros, the z + 1 bits of y + 1, the y low bits of l -- 2 z + 1 + y bits, and 3 more for the symbol;
* a block is 8 words of 64 bits.  It opens with the symbol counts of the block BEFORE it -- the total, then one count per symbol
  0..5 -- as 7 uint16 (total below 0x4000: type 0, 2 header words, 384 payload bits), 7 uint32 (below 2^30: type 1, 4 header
  words, 256 payload bits) or 7 uint64 (type 2, 7 header words, 64 payload bits), little endian; the type stands in bits 62-63
  of word 0.  Block 0 has an all-zero header of type 0;
* codes are written MSB first and may straddle two words of a block, never two blocks: the block that starts at run i holds the
  runs j with P[j + 1] - P[i] < C, where P is the prefix sum of the code widths and C the block's payload bits (a code that would
  reach the end of the last usable word opens the next block);
* blocks come in superblocks of 2^20; the last word of a superblock is never used, so its last block has 64 payload bits less;
* behind the data stands one more block of which only the header words (2, 4 or 7) are written.
"""
import array
import bisect
import collections
import concurrent.futures

import numpy as np

SB_BLOCKS = 1 << 20          # blocks per superblock
HDR_WORDS = (2, 4, 7)        # header words by block type
PAYLOAD = (384, 256, 64)     # payload bits by block type
SLAB = 1 << 21               # runs handled at a time (bounds the temporaries of chain and pack)

Chain = collections.namedtuple("Chain", "first_run type n_runs n_sym")


def ilog2(v):
    """floor(log2(v)) of positive integers below 2^62, exactly"""
    v = np.asarray(v, dtype=np.int64)
    assert v.size == 0 or (int(v.min()) >= 1 and int(v.max()) < (1 << 62)), "run lengths must be in [1, 2^62)"
    y = np.frexp(v.astype(np.float64))[1].astype(np.int64) - 1    # off by one only where the conversion rounded up to a power of two
    y -= (np.left_shift(np.int64(1), y) > v)
    return y


def widths(lens):
    """bits of the code of every run, symbol included"""
    lens = np.asarray(lens, dtype=np.int64)
    out = np.empty(lens.size, dtype=np.int64)
    for o in range(0, lens.size, SLAB):   # (a slab at a time: the temporaries stay in the cache)
        y = ilog2(lens[o:o + SLAB])
        out[o:o + SLAB] = 2 * ilog2(y + 1) + 1 + y + 3
    return out


def header_type(total):
    return 0 if total < 0x4000 else 1 if total < (1 << 30) else 2


def payload_bits(block, typ):
    return PAYLOAD[typ] - (64 if (block & (SB_BLOCKS - 1)) == SB_BLOCKS - 1 else 0)


def _prefix(a):
    p = np.zeros(a.size + 1, dtype=np.int64)
    np.cumsum(a, out=p[1:])
    return p


def chain(lens):
    """where the blocks begin: per block -- the trailing header-only one included, with no runs -- the first run, the header type,
    the number of runs and of symbols, as a Chain of four int64 arrays"""
    lens = np.asarray(lens, dtype=np.int64)
    n = lens.size
    assert n > 0
    P, S = _prefix(widths(lens)), _prefix(lens)
    first, typ = [], []
    i, t, b = 0, 0, 0
    while i < n:   # a slab of the prefix sums at a time as Python lists: one bisection per block
        s0, s1 = i, min(n, i + SLAB)
        Pl, Sl = array.array("q"), array.array("q")
        Pl.frombytes(P[s0:s1 + 1].tobytes()), Sl.frombytes(S[s0:s1 + 1].tobytes())
        while i < s1 and (s1 == n or i + 100 < s1):   # (a block spans fewer than 100 runs: it ends inside the slab)
            C = payload_bits(b, t)
            nx = s0 + bisect.bisect_left(Pl, Pl[i - s0] + C, i - s0 + 1, min(s1, i + C // 4) - s0 + 1) - 1   # the largest nx with P[nx] - P[i] < C
            if nx == i:
                raise ValueError("block %d (type %d) has no room for the code of run %d" % (b, t, i))
            first.append(i), typ.append(t)
            t = header_type(Sl[nx - s0] - Sl[i - s0])
            i, b = nx, b + 1
    first.append(n), typ.append(t)
    first = np.array(first, dtype=np.int64)
    n_runs = np.diff(np.concatenate([first, [n]]))
    return Chain(first, np.array(typ, dtype=np.int64), n_runs, S[np.concatenate([first[1:], [n]])] - S[first])


def _headers(words, ch, lens, syms):
    """the header of block b + 1 counts the symbols of block b"""
    nb = ch.first_run.size - 1
    cnt = np.zeros((7, nb), dtype=np.uint64)
    for c in range(6):
        cnt[c + 1] = np.add.reduceat(np.where(syms == c, lens, 0), ch.first_run[:nb]).astype(np.uint64)
    cnt[0] = cnt[1:].sum(axis=0)
    assert np.array_equal(cnt[0].astype(np.int64), ch.n_sym[:nb])
    base = (np.arange(1, nb + 1, dtype=np.int64)) * 8
    typ = ch.type[1:]
    u = np.uint64
    m = typ == 0
    words[base[m]] = cnt[0][m] | cnt[1][m] << u(16) | cnt[2][m] << u(32) | cnt[3][m] << u(48)
    words[base[m] + 1] = cnt[4][m] | cnt[5][m] << u(16) | cnt[6][m] << u(32)
    m = typ == 1
    for q in range(4):
        words[base[m] + q] = cnt[2 * q][m] | (cnt[2 * q + 1][m] << u(32) if q < 3 else u(0))
    m = typ == 2
    for q in range(7):
        words[base[m] + q] = cnt[q][m]
    words[base] |= typ.astype(np.uint64) << u(62)


def _pack_slab(words, ch, lens, syms, b0, b1):
    """the codes of blocks b0 .. b1 - 1 into their words"""
    u = np.uint64
    j0, j1 = int(ch.first_run[b0]), int(ch.first_run[b1])
    l, c = lens[j0:j1], syms[j0:j1].astype(np.uint64)
    y = ilog2(l)
    w = 2 * ilog2(y + 1) + 1 + y + 3
    yu = y.astype(np.uint64)
    x = ((l.astype(np.uint64) ^ (u(1) << yu)) | (yu + u(1)) << yu) << u(3) | c
    nr = ch.n_runs[b0:b1]
    P = _prefix(w)
    pos = np.repeat(np.arange(b0, b1, dtype=np.int64) * 512 + np.asarray(HDR_WORDS, dtype=np.int64)[ch.type[b0:b1]] * 64 - P[ch.first_run[b0:b1] - j0], nr) + P[:-1]
    end = (pos & 63) + w                         # bits of the word used behind this code
    wi = pos >> 6
    st = end > 64                                # the code straddles two words
    hi = np.where(st, x >> (np.maximum(end, 64) - 64).astype(np.uint64), x << (64 - np.minimum(end, 64)).astype(np.uint64))
    # every code gives one value for its word and, if it straddles, one for the next: in run order the words never go back
    k = np.arange(l.size, dtype=np.int64) + np.cumsum(st) - st
    ns = int(st.sum())
    vals, idx = np.zeros(l.size + ns, dtype=np.uint64), np.zeros(l.size + ns, dtype=np.int64)
    vals[k], idx[k] = hi, wi
    vals[k[st] + 1], idx[k[st] + 1] = x[st] << (128 - end[st]).astype(np.uint64), wi[st] + 1
    assert ((wi[st] + 1) >> 3 == pos[st] >> 9).all() and (end[~st] <= 64).all(), "a code left its block"
    starts = np.flatnonzero(np.concatenate([[True], idx[1:] != idx[:-1]]))
    assert (np.diff(idx[starts]) > 0).all()
    words[idx[starts]] |= np.bitwise_or.reduceat(vals, starts)


def pack(lens, syms, ch=None):
    """the word stream of the runs (lens[i] symbols syms[i]; neighbours must differ), as a uint64 array; ch: chain(lens) if at hand"""
    lens, syms = np.asarray(lens, dtype=np.int64), np.asarray(syms, dtype=np.uint8)
    assert lens.size == syms.size and int(syms.max()) <= 5 and not (syms[1:] == syms[:-1]).any(), "runs must be maximal, of symbols 0..5"
    if ch is None:
        ch = chain(lens)
    nb = ch.first_run.size - 1
    words = np.zeros(8 * nb + HDR_WORDS[int(ch.type[nb])], dtype=np.uint64)
    _headers(words, ch, lens, syms)
    slabs, b0 = [], 0
    while b0 < nb:   # slabs of whole blocks: their words are disjoint
        b1 = min(nb, max(b0 + 1, int(np.searchsorted(ch.first_run, ch.first_run[b0] + SLAB, side="right")) - 1))
        slabs.append((b0, b1))
        b0 = b1
    if len(slabs) == 1:
        _pack_slab(words, ch, lens, syms, *slabs[0])
    else:
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
            for f in [ex.submit(_pack_slab, words, ch, lens, syms, a, b) for a, b in slabs]:
                f.result()
    return words


def _block_runs(words, b, nwords):
    """the runs of block b as a list of (length, symbol)"""
    typ = int(words[8 * b]) >> 62
    if typ > 2:
        raise ValueError("block %d: type 3" % b)
    C = payload_bits(b, typ)
    lo, hi = 8 * b + HDR_WORDS[typ], min(nwords, 8 * b + HDR_WORDS[typ] + C // 64)
    v, nbits = 0, 64 * (hi - lo)
    for q in range(lo, hi):
        v = v << 64 | int(words[q])
    out = []
    while v:
        z = nbits - v.bit_length()                   # leading zeros: the class of y + 1
        wd = 2 * z + 1
        y = (v >> (nbits - wd)) - 1
        wd += y + 3
        if wd > nbits:
            raise ValueError("block %d: a code runs over the block's end" % b)
        code = v >> (nbits - wd)
        sym, l = code & 7, 1 << y | (code >> 3 & ((1 << y) - 1))
        if sym > 5:
            raise ValueError("block %d: symbol %d" % (b, sym))
        out.append((l, sym))
        nbits -= wd
        v &= (1 << nbits) - 1
    return out


def unpack(words):
    """the runs of a word stream: (lens, syms)"""
    words = np.asarray(words, dtype=np.uint64)
    lens, syms = [], []
    for b in range(words.size >> 3):
        for l, c in _block_runs(words, b, words.size):
            lens.append(l), syms.append(c)
    return np.array(lens, dtype=np.int64), np.array(syms, dtype=np.uint8)


def header_counts(words, b):
    """(type, [total, count of 0..5]) the header of block b states"""
    typ = int(words[8 * b]) >> 62
    raw = np.asarray(words[8 * b:8 * b + HDR_WORDS[min(typ, 2)]], dtype="<u8").copy()
    raw[0] &= np.uint64((1 << 62) - 1)
    return typ, raw.view(("<u2", "<u4", "<u8")[min(typ, 2)])[:7].astype(np.int64).tolist()


def describe(words_a, words_b, ch=None):
    """where two word streams part: the first differing block, its type, its runs and the word; ch: the chain of the runs, if at hand"""
    a, b = np.asarray(words_a, dtype=np.uint64), np.asarray(words_b, dtype=np.uint64)
    n = min(a.size, b.size)
    d = np.flatnonzero(a[:n] != b[:n])
    if d.size == 0:
        return "the streams agree" if a.size == b.size else "%d words against %d; the first %d agree" % (a.size, b.size, n)
    i = int(d[0])
    blk, q = i >> 3, i & 7
    ta, tb = int(a[8 * blk]) >> 62, int(b[8 * blk]) >> 62
    s = "%d words against %d, %d differ; the first in block %d (block %d of superblock %d), word %d (%s): %016x against %016x; block type %d against %d" % (
        a.size, b.size, d.size, blk, blk & (SB_BLOCKS - 1), blk >> 20, q, "header" if q < HDR_WORDS[min(tb, 2)] else "payload", int(a[i]), int(b[i]), ta, tb)
    if ch is not None and blk < ch.first_run.size:
        s += "; by the model the block holds runs %d..%d (%d symbols) behind a type-%d header" % (ch.first_run[blk], ch.first_run[blk] + ch.n_runs[blk] - 1, ch.n_sym[blk], ch.type[blk])
    for name, w in (("first", a), ("second", b)):
        try:
            r = _block_runs(w, blk, w.size) if 8 * blk + 8 <= w.size else []
            s += "; %s stream: %d runs in the block, %s ..." % (name, len(r), r[:4])
        except ValueError as e:
            s += "; %s stream: %s" % (name, e)
    return s


def runs_of_plain(plain):
    """(lens, syms) of the maximal runs of a BWT given one symbol per byte"""
    plain = np.asarray(plain, dtype=np.uint8)
    starts = np.concatenate([[0], np.flatnonzero(plain[1:] != plain[:-1]) + 1])
    return np.diff(np.concatenate([starts, [plain.size]])).astype(np.int64), plain[starts]


def expand(lens, syms):
    return np.repeat(np.asarray(syms, dtype=np.uint8), np.asarray(lens, dtype=np.int64))
