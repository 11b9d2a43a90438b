"""`fetch` restated in Python: the text-order table, the plan, the measuring pass and the walkers of rb3gpu_fetch over a plain BWT and the
sampled suffix array (S, ms, r2i, ssa) of its index, step by step as the kernels take them -- the symbols of every region and the exact n_walkers,
n_measured, n_steps and max_walk_steps of the call.

Test infrastructure only -- nothing under ropebwt3_amd/ imports this."""
import gzip
import struct

import numpy as np


class FetchInvalid(Exception):
    """an invalid region: .bad is the index of the first one (RB3GPU_EINVAL)"""

    def __init__(self, bad):
        Exception.__init__(self, "region %d is invalid" % bad)
        self.bad = bad


class FetchInconsistent(Exception):
    """a walker met a row the sampled suffix array does not describe (RB3GPU_EINTERNAL)"""


def read_ssa(path):
    """a .ssa file: (S, ms, r2i, ssa)"""
    with open(path, "rb") as f:
        b = f.read()
    assert b[:4] == b"SSA\1"
    ss, ms, m, n = struct.unpack("<IIqq", b[4:28])
    return ss, ms, np.frombuffer(b, dtype="<u8", count=m, offset=28).copy(), np.frombuffer(b, dtype="<u8", count=n, offset=28 + 8 * m).copy()


def read_bwt(path):
    """a plain BWT of $ACGTN letters (gzipped or not) as nt6 codes"""
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        s = f.read().strip()
    tab = np.full(256, 5, dtype=np.uint8)
    for i, c in enumerate(b"$ACGTN"):
        tab[c] = i
    return tab[np.frombuffer(s, dtype=np.uint8)]


class FetchModel:
    def __init__(self, bwt, S, ms, r2i, ssa):
        b = np.ascontiguousarray(bwt, dtype=np.uint8)
        cnt = np.bincount(b, minlength=6)
        acc = np.concatenate([[0], np.cumsum(cnt)])
        lf = np.zeros(b.size, dtype=np.int64)
        for c in range(6):
            idx = np.flatnonzero(b == c)
            lf[idx] = acc[c] + np.arange(idx.size)
        self.b, self.lf = b.tolist(), lf.tolist()              # one LF step from row k: symbol b[k], next row lf[k]
        self.m, self.n, self.S, self.ms = int(acc[1]), int(b.size), int(S), int(ms)
        self.mask = (1 << self.S) - 1
        self.ssa = [int(x) for x in ssa]
        assert len(self.ssa) == (self.n - self.m + self.mask) >> self.S and len(r2i) == self.m
        self.s = [x & ((1 << self.ms) - 1) for x in self.ssa]
        self.o = [x >> self.ms for x in self.ssa]
        # the table: the samples by (string, offset)
        self.tab = sorted(range(len(self.ssa)), key=lambda x: (self.s[x], self.o[x]))
        self.keys = [(self.s[x], self.o[x]) for x in self.tab]
        self._len = {}

    def _lower(self, r, o):
        lo, hi = 0, len(self.keys)
        while lo < hi:
            mid = (lo + hi) >> 1
            if self.keys[mid] < (r, o):
                lo = mid + 1
            else:
                hi = mid
        return lo

    def samples_of(self, r):
        """the offsets of the samples of string r, ascending"""
        return [self.keys[i][1] for i in range(self._lower(r, 0), self._lower(r + 1, 0))]

    def plan(self, r, beg, end):
        """(first, last, anchor): the inner walkers tab[first:last], the anchor as (row, offset) or None"""
        first, last = self._lower(r, beg + 1), self._lower(r, end)
        if last < len(self.keys) and self.keys[last][0] == r:
            x = self.tab[last]
            return first, last, (self.m + (x << self.S), self.o[x])
        return first, last, None

    def measure(self, r):
        """(length of string r, the steps of the measuring walk): from row r to the first sample's row or to the sentinel"""
        if r not in self._len:
            k, t = r, 0
            while True:
                c, k = self.b[k], self.lf[k]
                t += 1
                if c == 0:
                    self._len[r] = (t - 1, t)
                    break
                if ((k - self.m) & self.mask) == 0:
                    x = (k - self.m) >> self.S
                    if self.s[x] != r:
                        raise FetchInconsistent("measuring string %d met a sample of string %d" % (r, self.s[x]))
                    self._len[r] = (self.o[x] + t, t)
                    break
        return self._len[r]

    def _walk(self, r, k, o, beg, end, out):
        """one walker from (row k, offset o): its steps"""
        steps = 0
        while o > beg:
            c, k = self.b[k], self.lf[k]
            steps += 1
            if c == 0:
                raise FetchInconsistent("the start of string %d above offset %d" % (r, beg))
            o -= 1
            if o < end:
                assert out[o - beg] is None, "offset %d read twice" % o
                out[o - beg] = c
            if o == beg:
                break
            if ((k - self.m) & self.mask) == 0:
                x = (k - self.m) >> self.S
                if self.ssa[x] != (o << self.ms | r):
                    raise FetchInconsistent("row %d is not offset %d of string %d" % (k, o, r))
                break
        return steps

    def fetch(self, regions):
        """regions: (row, beg, end) triples.  (list of uint8 arrays, dict of n_walkers, n_measured, n_steps, max_walk_steps, anchor_offsets)"""
        plans, n_measured, n_steps, bad = [], 0, 0, None
        for i, (r, beg, end) in enumerate(regions):
            if not (0 <= r < self.m and 0 <= beg < end):
                bad = i if bad is None else bad
                plans.append(None)
                continue
            first, last, anchor = self.plan(r, beg, end)
            if anchor is None:
                length, t = self.measure(r)
                n_measured, n_steps = n_measured + 1, n_steps + t
                if end > length and bad is None:
                    bad = i
                anchor = (r, length)
            plans.append((first, last, anchor))
        if bad is not None:
            raise FetchInvalid(bad)
        seqs, n_walkers, max_walk, anchors = [], 0, 0, []
        for (r, beg, end), (first, last, anchor) in zip(regions, plans):
            out = [None] * (end - beg)
            walkers = [anchor] + [(self.m + (self.tab[i] << self.S), self.keys[i][1]) for i in range(first, last)]
            total = 0
            for k, o in walkers:
                st = self._walk(r, k, o, beg, end, out)
                assert st >= 1
                total, max_walk = total + st, max(max_walk, st)
            assert total == anchor[1] - beg, "the steps of a region sum to o_anchor - beg"
            assert None not in out
            n_walkers, n_steps = n_walkers + len(walkers), n_steps + total
            anchors.append(anchor[1])
            seqs.append(np.array(out, dtype=np.uint8))
        return seqs, {"n_walkers": n_walkers, "n_measured": n_measured, "n_steps": n_steps, "max_walk_steps": max_walk, "anchor_offsets": anchors}


def edge_regions(model, r, length):
    """the regions of string r (of `length` symbols) that the tests name, picked from the sorted table: {kind: (r, beg, end)}; a kind the string's samples
    do not offer is absent"""
    offs = model.samples_of(r)
    out = {"first": (r, 0, 1), "last": (r, length - 1, length), "whole": (r, 0, length)}
    for o in offs:
        if "beg_at_sample" not in out and 0 < o < length - 1:
            out["beg_at_sample"] = (r, o, min(o + 7, length))
        if "end_at_sample" not in out and o >= 2:
            out["end_at_sample"] = (r, max(o - 9, 0), o)
        if "end_above_sample" not in out and o >= 1 and o + 1 <= length:
            out["end_above_sample"] = (r, max(o - 5, 0), o + 1)
    for a, b in zip(offs, offs[1:]):
        if b - a >= 3:
            out["between_samples"] = (r, a + 1, b - 1)
            break
    top = offs[-1] if offs else -1
    if top + 1 < length:
        out["beyond_last_sample"] = (r, top + 1, min(top + 12, length))
    return out


EDGE_KINDS = ("first", "last", "whole", "beg_at_sample", "end_at_sample", "end_above_sample", "between_samples", "beyond_last_sample")
