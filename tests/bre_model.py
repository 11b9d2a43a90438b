"""The BRE interchange format restated in plain Python (bre.h of the reference): the independent model the host library,
the HIP packer / unpacker and the CLI are tested against.  Test infrastructure only.

File: "BRE\\1", b_per_sym (1), b_per_run, atype (2 = DNA6), mtype (0), asize (8 bytes LE, 6), l_aux (8 bytes LE), l_aux bytes;
records of one symbol byte and b_per_run length bytes (LE), a run longer than 2^(8 b_per_run) - 1 split into records of that
length and a remainder; one all-zero record; n_rec, n_sym, n_run (8 bytes LE each)."""
import numpy as np


def runs_of(bwt):
    """maximal runs [(symbol, length)] of a plain BWT (array of 0..5)"""
    b = np.asarray(bwt, dtype=np.uint8)
    if b.size == 0:
        return []
    cut = np.flatnonzero(np.diff(b)) + 1
    st = np.concatenate(([0], cut))
    en = np.concatenate((cut, [b.size]))
    return [(int(b[s]), int(e - s)) for s, e in zip(st, en)]


def join(runs):
    out = []
    for c, l in runs:
        if out and out[-1][0] == c:
            out[-1] = (c, out[-1][1] + l)
        else:
            out.append((c, l))
    return out


def records(runs, b_per_run=2, joined=True):
    """(record bytes, (n_rec, n_sym, n_run)) of a run list; joined=False: every record of more than one symbol is written as
    (c, 1), (c, l - 1) -- a writer that does not join records of one symbol, which a reader must accept"""
    mx = (1 << (8 * b_per_run)) - 1
    out, n_rec = bytearray(), 0
    runs = join(runs)
    for c, l in runs:
        rest = l
        while rest > 0:
            k = min(rest, mx)
            for part in ((1, k - 1) if (not joined and k > 1) else (k,)):
                out += bytes([c]) + part.to_bytes(b_per_run, "little")
                n_rec += 1
            rest -= k
    return bytes(out), (n_rec, sum(l for _, l in runs), len(runs))


def encode(runs, b_per_run=2, joined=True, aux=b""):
    """a whole BRE file"""
    rec, cnt = records(runs, b_per_run, joined)
    hdr = b"BRE\x01" + bytes([1, b_per_run, 2, 0]) + (6).to_bytes(8, "little") + len(aux).to_bytes(8, "little") + aux
    return hdr + rec + bytes(1 + b_per_run) + b"".join(x.to_bytes(8, "little") for x in cnt)


def decode(data):
    """(b_per_run, maximal runs, (n_rec, n_sym, n_run) as counted, the footer's three counts) of a whole BRE file"""
    assert data[:4] == b"BRE\x01" and data[4] == 1 and int.from_bytes(data[8:16], "little") == 6
    bpr, p = data[5], 24 + int.from_bytes(data[16:24], "little")
    runs, n_rec = [], 0
    while True:
        c, l = data[p], int.from_bytes(data[p + 1:p + 1 + bpr], "little")
        p += 1 + bpr
        if c == 0 and l == 0:
            break
        assert c <= 5 and l > 0
        runs.append((c, l))
        n_rec += 1
    runs = join(runs)
    ftr = tuple(int.from_bytes(data[p + 8 * i:p + 8 * i + 8], "little") for i in range(3))
    return bpr, runs, (n_rec, sum(l for _, l in runs), len(runs)), ftr


def plain_of(runs):
    return np.concatenate([np.full(l, c, dtype=np.uint8) for c, l in runs]) if runs else np.zeros(0, dtype=np.uint8)
