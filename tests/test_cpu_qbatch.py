"""the batch reader of the query commands (rb3h_qbatch_read, librb3host.so) without a device: whatever the batch size, the batches laid end to end
are the file as rb3h_seq_read1 gives it record by record -- nt6 codes, offsets, names --, a batch ends with the record that reaches the size or the
record count, too long a record is refused, a FASTX error ends the file behind its good records, and the buffers serve call after call."""
import ctypes
import os

import pytest

from ropebwt3_amd import host
from tests.test_cpu_mem import _read1_all

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64_MAX = (1 << 63) - 1
FILES = [("mem_mutated.fa.gz", False), ("mem_iupac.fa", False), ("reads_fq.fa.gz", False), ("edge_chars.txt", True), ("k4_readme.txt", True)]
TRUNCATED = b">r1 comment here\nACGT\nacgtn\n>r2\tx\n\n>\n>r3\r\nGG\r\nTT\r\n@q1 c\nACGTA\n+\nIIIII\n@q2\nAC\n+q2\nI\n"   # (the file of test_cpu_mem.test_reader_grammar)


class _QBatch(ctypes.Structure):
    _fields_ = [("sym", host._Buf), ("names", host._Buf), ("off", ctypes.POINTER(ctypes.c_int64)), ("name_off", ctypes.POINTER(ctypes.c_int64)),
                ("n", ctypes.c_int64), ("m", ctypes.c_int64), ("eof", ctypes.c_int)]


def _lib():
    L = host.load_library()
    L.rb3h_qbatch_read.restype = ctypes.c_int64
    L.rb3h_qbatch_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(_QBatch), ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    L.rb3h_qbatch_free.restype = None
    L.rb3h_qbatch_free.argtypes = [ctypes.POINTER(_QBatch)]
    L.rb3h_seq_error.restype = ctypes.c_int
    L.rb3h_seq_error.argtypes = [ctypes.c_void_p]
    L.rb3h_char2nt6.restype = None
    L.rb3h_char2nt6.argtypes = [ctypes.c_int64, ctypes.c_char_p]
    return L


def _nt6(s):
    buf = ctypes.create_string_buffer(s, len(s) + 1)
    _lib().rb3h_char2nt6(len(s), buf)
    return buf.raw[:len(s)]


def _caps(b):
    return (b.sym.m, b.sym.s, b.names.m, b.names.s, b.m, ctypes.cast(b.off, ctypes.c_void_p).value, ctypes.cast(b.name_off, ctypes.c_void_p).value)


def _batches(path, is_line, max_sym, max_rec=I64_MAX, max_len=I64_MAX, b=None):
    """every batch of the file as (records, symbols): records = [(name or None, nt6 codes)]; then the last return value and the reader's error code"""
    L = _lib()
    own = b is None
    b = _QBatch() if own else b
    fp = L.rb3h_seq_open(str(path).encode(), int(is_line))
    assert fp
    out, n = [], 0
    while n >= 0:
        n = L.rb3h_qbatch_read(fp, ctypes.byref(b), max_sym, max_rec, max_len)
        if n < 0:
            break
        assert n == b.n and (n == 0 or (b.off[0] == 0 and b.off[n] == b.sym.l and n + 1 <= b.m))
        sym = ctypes.string_at(b.sym.s, b.sym.l) if b.sym.l else b""
        names = ctypes.string_at(b.names.s, b.names.l) if b.names.l else b""
        recs = []
        for q in range(n):
            assert b.off[q] <= b.off[q + 1] and -1 <= b.name_off[q] < max(b.names.l, 0)
            nm = None if b.name_off[q] < 0 else names[b.name_off[q]:names.index(b"\0", b.name_off[q])].decode()
            recs.append((nm, sym[b.off[q]:b.off[q + 1]]))
        out.append(recs)
        if b.eof:
            break
    err = L.rb3h_seq_error(fp)
    L.rb3h_seq_close(fp)
    if own:
        L.rb3h_qbatch_free(ctypes.byref(b))
    return out, n, err


_TRUTH = {}


def _truth(name, is_line):
    if name not in _TRUTH:
        recs, err = _read1_all(os.path.join(GOLDEN, name), is_line)
        assert err == 0 and len(recs) > 0
        _TRUTH[name] = [(nm, _nt6(s)) for nm, s in recs]
    return _TRUTH[name]


@pytest.mark.parametrize("max_sym", [1, 1000, 10 ** 8])
@pytest.mark.parametrize("name,is_line", FILES)
def test_batches_are_the_file(name, is_line, max_sym):
    want = _truth(name, is_line)
    got, n, err = _batches(os.path.join(GOLDEN, name), is_line, max_sym)
    assert n >= 0 and err == 0
    assert [r for bt in got for r in bt] == want                       # symbols, offsets, names and the -1 of lines: all of the file, in order
    assert all((nm is None) == is_line for nm, _ in want)
    for bt in got[:-1]:                                                # a batch ends with the record that reaches max_sym
        total = sum(len(s) for _, s in bt)
        assert len(bt) > 0 and total >= max_sym and total - len(bt[-1][1]) < max_sym
    if max_sym == 10 ** 8:
        assert len(got) == 1
    if max_sym == 1:                                                   # (one record a batch, but for records of no symbols)
        assert len(got) >= sum(1 for _, s in want if len(s) > 0)


@pytest.mark.parametrize("name,is_line", FILES)
def test_record_cap(name, is_line):
    want = _truth(name, is_line)
    got, n, err = _batches(os.path.join(GOLDEN, name), is_line, 10 ** 8, max_rec=3)
    assert n >= 0 and err == 0 and [r for bt in got for r in bt] == want
    assert all(len(bt) == 3 for bt in got[:-1]) and len(got[-1]) <= 3 and len(got) >= (len(want) + 2) // 3


def test_empty_records_never_end_a_batch(tmp_path):
    p = tmp_path / "e.fa"
    p.write_bytes(b">a\n\n>b\n\n>c\nAC\n>d\n\n>e\nG\n>f\n\n")
    got, n, err = _batches(p, False, 1)
    assert err == 0 and got == [[("a", b""), ("b", b""), ("c", b"\1\2")], [("d", b""), ("e", b"\3")], [("f", b"")]]
    t = tmp_path / "e.txt"
    t.write_bytes(b"\n\nT\n\n")
    got, n, err = _batches(t, True, 1)
    assert err == 0 and got == [[(None, b""), (None, b""), (None, b"\4")], [(None, b"")]]
    got, n, err = _batches(t, True, 1, max_rec=2)                     # (the record cap counts them all the same)
    assert err == 0 and got == [[(None, b""), (None, b"")], [(None, b"\4")], [(None, b"")]]


def test_too_long_a_record(tmp_path):
    p = tmp_path / "l.fa"
    p.write_bytes(b">a\nACGTACGTAC\n>b\nACGTACGTACG\n>c\nA\n")
    got, n, err = _batches(p, False, 10 ** 8, max_len=10)
    assert n == -2 and got == []
    got, n, err = _batches(p, False, 1, max_len=10)                   # (the batch before it is whole)
    assert n == -2 and got == [[("a", _nt6(b"ACGTACGTAC"))]]
    got, n, err = _batches(p, False, 10 ** 8, max_len=11)
    assert n == 3 and err == 0 and [len(s) for _, s in got[0]] == [10, 11, 1]


@pytest.mark.parametrize("max_sym", [1, 10 ** 8])
def test_fastx_error_behind_the_good_records(tmp_path, max_sym):
    p = tmp_path / "a.fa"
    p.write_bytes(TRUNCATED)
    got, n, err = _batches(p, False, max_sym)
    assert [r for bt in got for r in bt] == [("r1", _nt6(b"ACGTacgtn")), ("r2", b""), ("", b""), ("r3", _nt6(b"GGTT")), ("q1", _nt6(b"ACGTA"))]
    assert n >= 0 and err == -2                                         # (_batches stops at eof: the error is what ended the file)
    assert [len(bt) for bt in got] == ([5] if max_sym > 1 else [1, 3, 1, 0])        # (q1 reached the size: the end of the file is the next call's to find)


def test_buffers_are_reused_and_freed(tmp_path):
    L = _lib()
    b = _QBatch()
    assert bytes(b) == bytes(ctypes.sizeof(b))
    big = _batches(os.path.join(GOLDEN, "mem_mutated.fa.gz"), False, 10 ** 8, b=b)
    caps = _caps(b)
    assert big[0] and b.eof == 1 and all(caps)
    p = tmp_path / "small.fa"                                            # smaller in every way: fewer records, fewer symbols, shorter names
    p.write_bytes(b">x\nACGT\n")
    small = _batches(p, False, 10 ** 8, b=b)
    assert small[0] == [[("x", b"\1\2\3\4")]] and _caps(b) == caps and b.n == 1 and b.sym.l == 4 and b.names.l == 2
    again = _batches(os.path.join(GOLDEN, "mem_mutated.fa.gz"), False, 1000, b=b)
    assert [r for bt in again[0] for r in bt] == big[0][0] and _caps(b) == caps
    L.rb3h_qbatch_free(ctypes.byref(b))
    assert bytes(b) == bytes(ctypes.sizeof(b))
    L.rb3h_qbatch_free(ctypes.byref(b))                                # (and an empty one is freed without harm)
