"""A callback that stops a query driver in mid-call: every driver that streams to a callback is called through the C entry point with a
callback that returns 7 at its second invocation.  The call returns that 7 (every driver hands back what its callback said), the callback
is not invoked a third time, and the handle -- whose call left by an early return with grown buffers live -- then gives the full recorded
answer through the ordinary method of gpu.py, still in the small slices of the case."""
import ctypes
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

from ropebwt3_amd import _build, Rb3Gpu, gpu, host
from tests import kount_model as km
from tests import mem_model as mm
from tests import pos_model as pm
from tests import util

CLI = _build.BIN_CLI
GOLDEN = util.GOLDEN
STOP = 7


def _manifest(name, key):
    return json.load(open(os.path.join(GOLDEN, name)))[key]


@pytest.fixture(scope="module")
def h():
    """genomes12.fmd with its sampled suffix array (-s8), loaded once for all the cases; every case puts the tunes it set back to 0"""
    e = Rb3Gpu(verbose=1)
    e.from_plain(km.golden_plain(GOLDEN, "genomes12.fmd", CLI))
    e.set_ssa(*gpu.read_ssa(os.path.join(GOLDEN, "genomes12.s8.ssa")))
    yield e
    e.close()


@pytest.fixture(scope="module")
def strings():
    """the 24 strings of genomes12.fmd as genomes12.fa.gz records them: string 2i is sequence i, string 2i + 1 its reverse complement (nt6 codes)"""
    seqs = []
    for line in gzip.open(os.path.join(GOLDEN, "genomes12.fa.gz"), "rt"):
        if line.startswith(">"):
            seqs.append([])
        else:
            seqs[-1].append(line.strip())
    out = []
    for s in seqs:
        f = gpu.nt6_of("".join(s))
        out += [f, util.revcomp(f)]
    return out


def _stopper(ftype):
    """a callback of type ftype that says STOP from its second invocation on, and the count of its invocations"""
    calls = [0]

    def cb(*_args):
        calls[0] += 1
        return STOP if calls[0] >= 2 else 0
    return ftype(cb), calls


def _batch(queries):
    qs = [gpu.nt6_of(q) for q in queries]
    off = np.zeros(len(qs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([q.size for q in qs])
    return off, np.ascontiguousarray(np.concatenate(qs), dtype=np.uint8)


def _stopped(r, calls, full_slices):
    assert full_slices >= 3, full_slices     # (the full call makes a third callback: the stop is what keeps it from happening)
    assert r == STOP and calls[0] == 2, (r, calls[0])


def _eq(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_kount(h):
    e = _manifest("KOUNT_MANIFEST.json", "-k31 -m2 genomes12.fmd")
    cb, calls = _stopper(gpu.KOUNT_F)
    arr = (ctypes.c_void_p * 1)(h._h)
    r = h._lib.rb3gpu_kount(arr, 1, 31, 2, 1000, cb, None, None)     # a frontier of 1000 nodes: the levels grow as the walk descends, the output in many slices
    st = {}
    kmers, counts = h.kount(31, 2, max_level_nodes=1000, stats=st)
    _stopped(r, calls, st["n_slices"])
    out = gpu.kount_lines(kmers, counts)
    assert out.count(b"\n") == e["lines"] and hashlib.md5(out).hexdigest() == e["md5"]


@pytest.mark.gpu
def test_locate(h):
    """rb3gpu_locate has no tune: its slices are 2^20 intervals (or 2^21 pairs), so three slices take more than 2^21 intervals.  All but a few are
    empty (lo = hi: no pair, nothing walked); the first slice has 10 rows to locate and the second 100, so the pairs are regrown before the stop"""
    e = _manifest("MEMPOS_MANIFEST.json", "-s8 -l5 -c2 -p20 genomes12.fmd mem_mutated.fa.gz")
    a1, n = int(h.get_acc()[1]), (2 << 20) + 5
    lo = np.full(n, a1, dtype=np.int64)
    hi = lo.copy()
    lo[:10] += np.arange(10)
    hi[:10] = lo[:10] + 1
    lo[1 << 20:(1 << 20) + 100] += np.arange(100)
    hi[1 << 20:(1 << 20) + 100] = lo[1 << 20:(1 << 20) + 100] + 1
    cb, calls = _stopper(gpu.LOCATE_F)
    r = h._lib.rb3gpu_locate(h._h, n, lo.ctypes.data, hi.ctypes.data, 5, cb, None, None)
    st = {}
    off, pos = h.locate(lo, hi, 5, stats=st)
    _stopped(r, calls, st["n_slices"])
    assert off[-1] == pos.size == 110
    # the recorded answer: the positions of the matches of `mem -p20`, located here interval by interval
    qq = mm.read_queries(os.path.join(GOLDEN, "mem_mutated.fa.gz"))
    names, lengths = pm.read_len_gz(os.path.join(GOLDEN, "genomes12.len.gz"))
    recs = h.mem([s for _, s in qq], 5, 2)
    off, pos = h.locate(recs["x0"], recs["x0"] + recs["size"], 20)
    assert hashlib.md5(gpu.mem_lines(recs, [n for n, _ in qq], positions=(off, pos), seq_names=names, lengths=lengths)).hexdigest() == e["md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("max_pos", [0, 20])
def test_mem_and_mem_pos(h, max_pos):
    key = "-l5 -c2 genomes12.fmd mem_mutated.fa.gz" if max_pos == 0 else "-s8 -l5 -c2 -p20 genomes12.fmd mem_mutated.fa.gz"
    e = _manifest("MEM_MANIFEST.json" if max_pos == 0 else "MEMPOS_MANIFEST.json", key)
    qq = mm.read_queries(os.path.join(GOLDEN, "mem_mutated.fa.gz"))
    qs, qn = [s for _, s in qq], [n for n, _ in qq]
    off, sym = _batch(qs)
    names, lengths = pm.read_len_gz(os.path.join(GOLDEN, "genomes12.len.gz"))
    h.tune("mem_slice", 3000)     # output slices of 3000 query symbols, walkers of 64
    try:
        st = {}
        if max_pos == 0:
            cb, calls = _stopper(gpu.MEM_F)
            r = h._lib.rb3gpu_mem(h._h, len(qs), off.ctypes.data, sym.ctypes.data, 5, 2, 64, cb, None, None)
            recs = h.mem(qs, 5, 2, chunk=64, stats=st)
            out = gpu.mem_lines(recs, qn)
        else:
            cb, calls = _stopper(gpu.MEM_POS_F)
            r = h._lib.rb3gpu_mem_pos(h._h, len(qs), off.ctypes.data, sym.ctypes.data, 5, 2, 64, max_pos, cb, None, None, None)
            recs, poff, pos = h.mem(qs, 5, 2, chunk=64, max_pos=max_pos, stats=st)
            out = gpu.mem_lines(recs, qn, positions=(poff, pos), seq_names=names, lengths=lengths)
        _stopped(r, calls, st["n_slices"])
        assert out.count(b"\n") == e["lines"] and hashlib.md5(out).hexdigest() == e["md5"]
    finally:
        h.tune("mem_slice", 0)


@pytest.mark.gpu
def test_hapdiv(h):
    e = _manifest("HAPDIV_MANIFEST.json", "-a51 -w10 -N5 genomes12.fmd mem_mutated.fa.gz")
    qq = mm.read_queries(os.path.join(GOLDEN, "mem_mutated.fa.gz"))
    qs = [gpu.nt6_of(s) for _, s in qq]
    off, sym = _batch(qs)
    win = np.ascontiguousarray([off[i] + x for i, q in enumerate(qs) for x in range(0, q.size - 51 + 1, 10)], dtype=np.int64)
    opt = gpu.HapdivOpt(5, 30, 1, 3, 5, 2, -1)
    h.tune("hapdiv_slice", 500)
    try:
        cb, calls = _stopper(gpu.HAPDIV_F)
        r = h._lib.rb3gpu_hapdiv(h._h, win.size, win.ctypes.data, sym.ctypes.data, 51, ctypes.byref(opt), cb, None, None)
        st = {}
        recs, where = h.hapdiv(qs, 51, 10, n_best=5, stats=st)
        _stopped(r, calls, st["n_slices"])
        assert np.array_equal(off[where[:, 0]] + where[:, 1], win)
        assert hashlib.md5(gpu.hapdiv_lines(recs, where, 51, [n for n, _ in qq])).hexdigest() == e["md5"]
    finally:
        h.tune("hapdiv_slice", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("local", [False, True])
def test_sw_e2e_and_sw_local(h, local):
    e = _manifest("SWLOCAL_MANIFEST.json", "-s8 -p3 genomes12.fmd sw_reads.fa") if local else _manifest("SW_MANIFEST.json", "-s8 -e -p3 genomes12.fmd sw_reads.fa")
    qq = mm.read_queries(os.path.join(GOLDEN, "sw_reads.fa"))
    qs, qn = [s for _, s in qq], [n for n, _ in qq]
    off, sym = _batch(qs)
    names, lengths = pm.read_len_gz(os.path.join(GOLDEN, "genomes12.len.gz"))
    h.tune("sw_slice", 40)
    try:
        cb, calls = _stopper(gpu.SW_F)
        st = {}
        if local:
            g = host.dawg_batch(off, sym)
            node_off, nsym = np.ascontiguousarray(g["node_off"], dtype=np.int64), np.ascontiguousarray(g["sym"], dtype=np.uint8)
            pre_off, pre = np.ascontiguousarray(g["pre_off"], dtype=np.int64), np.ascontiguousarray(g["pre"], dtype=np.int32)
            hit_node = np.full(len(qs), -1, dtype=np.int32)
            opt = gpu.SwOpt(25, 30, 1, 3, 5, 2, -1, 11, 3)
            r = h._lib.rb3gpu_sw_local(h._h, len(qs), off.ctypes.data, sym.ctypes.data, node_off.ctypes.data, nsym.ctypes.data, pre_off.ctypes.data, pre.ctypes.data,
                                       ctypes.byref(opt), cb, None, hit_node.ctypes.data, None, None)
            hits = h.sw_local(qs, max_pos=3, stats=st, dawg=g)
        else:
            opt = gpu.SwOpt(25, 30, 1, 3, 5, 2, -1, 1, 3)
            r = h._lib.rb3gpu_sw_e2e(h._h, len(qs), off.ctypes.data, sym.ctypes.data, ctypes.byref(opt), cb, None, None, None)
            hits = h.sw_e2e(qs, max_pos=3, stats=st)
        _stopped(r, calls, st["n_slices"])
        out = gpu.sw_lines(qs, hits, qn, seq_names=names, lengths=lengths)
        assert out.count(b"\n") == e["lines"] and hashlib.md5(out).hexdigest() == e["md5"]
    finally:
        h.tune("sw_slice", 0)


def _short_then_long(h):
    """three rows whose answers grow -- two rows inside strings (`get` spells what lies in front of a row's suffix) and a sentinel's row, a whole string --
    and the length of the first: with that as the budget the first row is a slice that fits and each of the others a slice of its own that exceeds
    it, so the output is regrown for the second callback"""
    a1 = int(h.get_acc()[1])
    cand = [a1 + 997 * j for j in range(1, 40)]
    _, seqs = h.retrieve(cand)
    by_len = sorted((s.size, k) for s, k in zip(seqs, cand) if s.size > 0)
    (n0, r0), (n1, r1) = by_len[0], by_len[len(by_len) // 2]
    assert 0 < n0 < n1 < 20000
    return np.ascontiguousarray([r0, r1, 0], dtype=np.int64), n0


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [False, True])
def test_retrieve_and_retrieve_pieces(h, strings, pieces):
    rows, budget = _short_then_long(h)
    h.tune("get_slice", budget)
    try:
        cb, calls = _stopper(gpu.RETRIEVE_F)
        r = (h._lib.rb3gpu_retrieve_pieces if pieces else h._lib.rb3gpu_retrieve)(h._h, rows.size, rows.ctypes.data, cb, None, None)
        _stopped(r, calls, rows.size)     # (every row a slice)
        end, seqs = h.retrieve(range(len(strings)), pieces=pieces)
        assert _eq(seqs, strings) and len(set(end.tolist())) == len(strings)
    finally:
        h.tune("get_slice", 0)


@pytest.mark.gpu
def test_fetch(h, strings):
    reg = np.ascontiguousarray([(3, 10, 110), (8, 0, 5000), (1, 5, strings[1].size - 3)], dtype=np.int64)     # 100 symbols, then 5000, then nearly a whole string
    bad = ctypes.c_int64(-1)
    h.tune("fetch_slice", 100)     # the first region fits, the others exceed it
    try:
        cb, calls = _stopper(gpu.FETCH_F)
        r = h._lib.rb3gpu_fetch(h._h, reg.shape[0], reg.ctypes.data, ctypes.byref(bad), cb, None, None)
        assert bad.value == -1
        _stopped(r, calls, reg.shape[0])     # (every region a slice)
        rng = np.random.default_rng(3)
        full = [(k, 0, s.size) for k, s in enumerate(strings)]
        for k, s in enumerate(strings):
            b = int(rng.integers(0, s.size - 70))
            full.append((k, b, b + int(rng.integers(1, 70))))
        a = np.array(full, dtype=np.int64)
        seqs = h.fetch(a[:, 0], a[:, 1], a[:, 2])
        assert _eq(seqs, [strings[k][b:e] for k, b, e in full])
    finally:
        h.tune("fetch_slice", 0)
