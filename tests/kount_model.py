"""Python model of `kount` (k-mer counting over one or more indexes), written from its semantics rather than from the trie walk:

- the strings of an index come from inverting its plain BWT (LF from every sentinel row back to the next sentinel);
- a k-mer is k consecutive symbols of one string, all of them A C G T (so none holds $ or N, none crosses a string end);
- a k-mer is reported if its count in SOME index is at least m (every one of the 4^k k-mers for m <= 0), with its count in every index;
- the order: the last character descending, then the one before it descending, ..., the first character ascending (the reference's
  stack pops the last child pushed, and prints the children of the last level in the loop's order)."""
import gzip
import itertools
import os
import subprocess

import numpy as np

LUT = bytes.maketrans(b"$ACGTN", bytes(range(6)))


def read_plain(path):
    """a plain BWT file ($ACGTN text, .gz or not) as symbols 0..5"""
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        s = f.read().replace(b"\n", b"")
    return np.frombuffer(s.translate(LUT), dtype=np.uint8)


def plain_of_index(path, cli):
    """the plain BWT of an FMD / FMR file, decoded on the host by the CLI's `recode`"""
    r = subprocess.run([cli, "recode", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, check=True)
    return np.frombuffer(r.stdout.replace(b"\n", b"").translate(LUT), dtype=np.uint8)


def strings_of(bwt):
    """the strings of a multi-string BWT (every one ends in a sentinel), each as a symbol array without its sentinel"""
    b = np.asarray(bwt, dtype=np.uint8)
    cnt = np.bincount(b, minlength=6)
    C = np.concatenate([[0], np.cumsum(cnt)])
    lf = np.empty(b.size, dtype=np.int64)
    for c in range(6):
        pos = np.flatnonzero(b == c)
        lf[pos] = C[c] + np.arange(pos.size)
    m = int(cnt[0])
    rows = np.arange(m, dtype=np.int64)  # row i: the sentinel of string i sorts as the i-th suffix; B there is its last symbol
    ids = np.arange(m)
    got_id, got_step, got_sym = [], [], []
    step = 0
    while rows.size:
        s = b[rows]
        live = s != 0
        rows, ids, s = rows[live], ids[live], s[live]
        got_id.append(ids), got_step.append(np.full(ids.size, step)), got_sym.append(s)
        rows = lf[rows]
        step += 1
    gid, gstep, gsym = np.concatenate(got_id), np.concatenate(got_step), np.concatenate(got_sym)
    o = np.lexsort((-gstep, gid))  # by string, first symbol first
    return np.split(gsym[o], np.cumsum(np.bincount(gid, minlength=m))[:-1])


def kmer_counts(strings, k):
    """(the distinct k-mers, symbols 1..4, as uint8 (n, k); their occurrences) over all strings"""
    wins = []
    for s in strings:
        if s.size < k:
            continue
        w = np.lib.stride_tricks.sliding_window_view(s, k)
        w = w[np.all((w >= 1) & (w <= 4), axis=1)]
        if w.size:
            wins.append(np.ascontiguousarray(w))
    if not wins:
        return np.zeros((0, k), dtype=np.uint8), np.zeros(0, dtype=np.int64)
    w = np.concatenate(wins)
    u, c = np.unique(w.view(np.dtype((np.void, k))).ravel(), return_counts=True)
    return np.frombuffer(u.tobytes(), dtype=np.uint8).reshape(-1, k), c.astype(np.int64)


def order(kmers):
    """the permutation that puts k-mers into the reference's output order"""
    kmers = np.asarray(kmers, dtype=np.int64)
    key = np.concatenate([5 - kmers[:, :0:-1], kmers[:, :1]], axis=1)  # last character descending, ..., first ascending
    return np.lexsort(key.T[::-1])


def kount(bwts, k, m):
    """(kmers uint8 (N, k), counts int64 (N, len(bwts))) of the indexes whose plain BWTs are `bwts`, in the reference's order"""
    return kount_strings([strings_of(b) for b in bwts], k, m)


def strings_of_text(text):
    """the strings of a text in which every string ends in 0"""
    text = np.asarray(text, dtype=np.uint8)
    ends = np.flatnonzero(text == 0)
    return np.split(text, ends + 1)[:-1] if ends.size else []


def kount_strings(collections, k, m):
    """kount over indexes given by their strings (one list of symbol arrays per index)"""
    per = [kmer_counts(c, k) for c in collections]
    if m <= 0:
        allk = np.array(list(itertools.product(range(1, 5), repeat=k)), dtype=np.uint8).reshape(-1, k)
        per_all = per + [(allk, np.zeros(allk.shape[0], dtype=np.int64))]
    else:
        per_all = per
    km = np.concatenate([p[0] for p in per_all])
    which = np.concatenate([np.full(p[0].shape[0], i) for i, p in enumerate(per_all)]).astype(np.int64)
    cn = np.concatenate([p[1] for p in per_all])
    if km.shape[0] == 0:
        return np.zeros((0, k), dtype=np.uint8), np.zeros((0, len(per)), dtype=np.int64)
    u, inv = np.unique(np.ascontiguousarray(km).view(np.dtype((np.void, k))).ravel(), return_inverse=True)
    keys = np.frombuffer(u.tobytes(), dtype=np.uint8).reshape(-1, k)
    counts = np.zeros((keys.shape[0], len(per_all)), dtype=np.int64)
    np.add.at(counts, (inv.ravel(), which), cn)
    counts = counts[:, :len(per)]
    if m > 0:
        keep = counts.max(axis=1) >= m
        keys, counts = keys[keep], counts[keep]
    o = order(keys)
    return np.ascontiguousarray(keys[o]), np.ascontiguousarray(counts[o])


def lines(kmers, counts):
    """the reference's output bytes"""
    lut = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    return b"".join(lut[s].tobytes() + b"".join(b"\t%d" % x for x in c) + b"\n" for s, c in zip(np.asarray(kmers, dtype=np.uint8), counts))


def golden_plain(golden_dir, name, cli):
    """the plain BWT of golden index `name` (file name with .fmd / .fmr): its .bwt.gz where there is one, else decoded by the CLI"""
    base = os.path.splitext(name)[0]
    p = os.path.join(golden_dir, base + ".bwt.gz")
    if os.path.exists(p):
        return read_plain(p)
    return plain_of_index(os.path.join(golden_dir, name), cli)
