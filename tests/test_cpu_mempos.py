"""mem -p without a GPU: the readers of the two side files (rb3h_ssa_read, rb3h_sid_read), the formatter of the position columns, the string
model of tests/pos_model.py pinned on recorded reference lines, what the manifest must hold, and the new symbols of the C ABI."""
import ctypes
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, gpu, host
from tests import kount_model as km
from tests import mem_model as mm
from tests import pos_model as pm

CLI = _build.BIN_CLI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MEMPOS_MANIFEST.json")))


class Ssa(ctypes.Structure):
    _fields_ = [("ss", ctypes.c_int32), ("ms", ctypes.c_int32), ("m", ctypes.c_int64), ("n_ssa", ctypes.c_int64), ("r2i", ctypes.POINTER(ctypes.c_uint64)), ("ssa", ctypes.POINTER(ctypes.c_uint64))]


class Sid(ctypes.Structure):
    _fields_ = [("n_seq", ctypes.c_int64), ("name", ctypes.POINTER(ctypes.c_char_p)), ("len", ctypes.POINTER(ctypes.c_int64))]


class Buf(ctypes.Structure):
    _fields_ = [("l", ctypes.c_int64), ("m", ctypes.c_int64), ("s", ctypes.c_void_p)]


def _lib():
    lib = host.load_library()
    lib.rb3h_ssa_read.restype = ctypes.POINTER(Ssa)
    lib.rb3h_ssa_read.argtypes = [ctypes.c_char_p]
    lib.rb3h_ssa_destroy.argtypes = [ctypes.POINTER(Ssa)]
    lib.rb3h_ssa_destroy.restype = None
    lib.rb3h_sid_read.restype = ctypes.POINTER(Sid)
    lib.rb3h_sid_read.argtypes = [ctypes.c_char_p]
    lib.rb3h_sid_destroy.argtypes = [ctypes.POINTER(Sid)]
    lib.rb3h_sid_destroy.restype = None
    lib.rb3h_mem_format_pos.restype = ctypes.c_int
    lib.rb3h_mem_format_pos.argtypes = [ctypes.POINTER(Buf), ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Sid)]
    return lib


@pytest.mark.parametrize("name,ss", [("genomes12.s8.ssa", 8), ("k3_both.s0.ssa", 0), ("reads_fwd.s3.ssa", 3)])
def test_ssa_read_golden_and_truncated(name, ss, tmp_path):
    lib = _lib()
    fn = os.path.join(GOLDEN, name)
    raw = open(fn, "rb").read()
    p = lib.rb3h_ssa_read(fn.encode())
    assert bool(p)
    sa = p.contents
    s2, ms, r2i, ssa = gpu.read_ssa(fn)
    assert (sa.ss, sa.ms, sa.m, sa.n_ssa) == (ss, ms, r2i.size, ssa.size) and s2 == ss
    assert len(raw) == 28 + 8 * (sa.m + sa.n_ssa)
    assert np.array_equal(np.ctypeslib.as_array(sa.r2i, shape=(sa.m,)), r2i)
    if sa.n_ssa:
        assert np.array_equal(np.ctypeslib.as_array(sa.ssa, shape=(sa.n_ssa,)), ssa)
    assert sorted(r2i.tolist()) == list(range(sa.m))          # a permutation of the strings
    lib.rb3h_ssa_destroy(p)
    for cut, what in ((len(raw) - 1, "last byte"), (28 + 8 * r2i.size - 3, "inside r2i"), (27, "header"), (3, "magic"), (0, "empty")):
        t = tmp_path / ("cut%d.ssa" % cut)
        t.write_bytes(raw[:cut])
        assert not lib.rb3h_ssa_read(str(t).encode()), what
    t = tmp_path / "magic.ssa"
    t.write_bytes(b"SSA\2" + raw[4:])
    assert not lib.rb3h_ssa_read(str(t).encode())
    assert not lib.rb3h_ssa_read(str(tmp_path / "missing.ssa").encode())


def test_sid_read_fields(tmp_path):
    lib = _lib()
    text = b"a\t10\nb 20 extra words\nonefield\nzero\t0\nneg\t-4\nc\t30\textra\nd  5\n\ne\t7x\nlast\t99"
    want = [(b"a", 10), (b"b", 20), (b"c", 30), (b"e", 7), (b"last", 99)]   # one field, length <= 0, an empty second field ("d  5"), an empty line: skipped
    for fn, data in (("plain.len", text), ("packed.len.gz", gzip.compress(text))):
        t = tmp_path / fn
        t.write_bytes(data)
        p = lib.rb3h_sid_read(str(t).encode())
        assert bool(p)
        s = p.contents
        assert [(s.name[i], s.len[i]) for i in range(s.n_seq)] == want
        lib.rb3h_sid_destroy(p)
    assert not lib.rb3h_sid_read(str(tmp_path / "missing.len.gz").encode())
    p = lib.rb3h_sid_read(os.path.join(GOLDEN, "genomes12.len.gz").encode())
    s = p.contents
    assert s.n_seq == 12 and [s.name[i] for i in range(12)] == [b"seq%d" % i for i in range(12)] and all(s.len[i] == 20000 for i in range(12))
    lib.rb3h_sid_destroy(p)


def test_format_pos_hand_written(tmp_path):
    lib = _lib()
    t = tmp_path / "x.len.gz"
    t.write_bytes(gzip.compress(b"chrA\t100\nchrB\t50\n"))
    sid = lib.rb3h_sid_read(str(t).encode())
    recs = np.zeros(4, dtype=gpu.MEM_REC)
    recs["st"], recs["en"], recs["size"] = [0, 5, 7, 30], [10, 25, 8, 31], [3, 1, 0, 9]
    off = np.array([0, 3, 4, 4, 6], dtype=np.int64)
    pos = np.array([(0, 5), (1, 5), (3, 0), (2, 40), (1, 99), (3, 49)], dtype=gpu.POS)
    out = Buf(0, 0, None)
    assert lib.rb3h_mem_format_pos(ctypes.byref(out), b"q1", 0, 4, recs.ctypes.data, off.ctypes.data, pos.ctypes.data, sid) == 0
    got = ctypes.string_at(out.s, out.l)
    want = (b"q1\t0\t10\t3\t3\tchrA:+:5\tchrA:-:85\tchrB:-:40\n"      # 100 - (5 + 10), 50 - (0 + 10)
            b"q1\t5\t25\t1\t1\tchrB:+:40\n"
            b"q1\t7\t8\t0\n"                                          # no positions: no extra column
            b"q1\t30\t31\t9\t2\tchrA:-:0\tchrB:-:0\n")                # 100 - (99 + 1), 50 - (49 + 1)
    assert got == want
    assert gpu.mem_lines(recs, names=["q1"], positions=(off, pos), seq_names=["chrA", "chrB"], lengths=[100, 50]) == want
    out2 = Buf(0, 0, None)
    assert lib.rb3h_mem_format_pos(ctypes.byref(out2), None, 6, 1, recs.ctypes.data, off.ctypes.data, pos.ctypes.data, sid) == 0
    assert ctypes.string_at(out2.s, out2.l).startswith(b"seq7\t0\t10\t3\t3\t")
    bad = np.array([(4, 0)], dtype=gpu.POS)   # a string the name list does not know
    assert lib.rb3h_mem_format_pos(ctypes.byref(out2), b"q", 0, 1, recs.ctypes.data, np.array([0, 1], dtype=np.int64).ctypes.data, bad.ctypes.data, sid) < 0
    lib.rb3h_sid_destroy(sid)


def test_manifest_shape():
    assert len(MANIFEST) >= 90
    assert {e["S"] for e in MANIFEST.values()} >= {0, 3, 8}
    assert {e["files"][0] for e in MANIFEST.values()} >= {"genomes12.fmd", "copies3000.fmd", "edge_dups.fmd", "longruns.fmd", "k4_readme.fmd"}
    for k, e in MANIFEST.items():
        assert os.path.exists(os.path.join(GOLDEN, e["len"])) and re.fullmatch(r"[0-9a-f]{32}", e["md5"]) and any(o.startswith("-p") for o in e["opts"]), k
        assert e["ssa"] is None or os.path.exists(os.path.join(GOLDEN, e["ssa"]))
    for S in (0, 3, 8):   # the cases of the issue's table
        assert MANIFEST["-s%d -l19 -p5 genomes12.fmd mem_mutated.fa.gz" % S]["lines"] == 418
        assert MANIFEST["-s%d -l5 -c2 -p20 genomes12.fmd mem_mutated.fa.gz" % S]["max_size"] == 154
        assert MANIFEST["-s%d -l31 -p10 genomes12.fmd mem_iupac.fa" % S]["lines"] == 10
    assert MANIFEST["-s8 -l5 -c2 -p20 genomes12.fmd reads_fq.fa.gz"]["lines"] == 175369
    a, b = (MANIFEST["-s%d -l5 -c2 -p20 genomes12.fmd mem_mutated.fa.gz" % S]["md5"] for S in (3, 8))
    assert a != b                                              # the sample rate decides which occurrences a capped line holds
    for f in os.listdir(GOLDEN):                               # no side file under a name `mem -p <golden index>` would find
        assert not any(f == i + suf for i in os.listdir(GOLDEN) if i.endswith((".fmd", ".fmr")) for suf in (".ssa", ".len.gz")), f


@pytest.mark.parametrize("key", sorted(k for k, e in MANIFEST.items() if "out" in e and e["files"][0] in ("genomes12.fmd", "edge_dups.fmd", "k4_readme.fmd", "k3_both.fmd")))
def test_model_on_recorded_lines(key):
    """every recorded line: its columns are distinct, min(P, size) of them, and all of them occurrences of the match according to the strings;
    all the occurrences where the cap admits them"""
    e = MANIFEST[key]
    strings = mm.index_strings(GOLDEN, e["files"][0], CLI)
    names, lengths = pm.read_len_gz(os.path.join(GOLDEN, e["len"]))
    assert 2 * len(names) == len(strings)
    P = [int(o[2:]) for o in e["opts"] if o.startswith("-p")][0]
    queries = []
    for f in e["files"][1:]:
        queries += mm.read_queries(os.path.join(GOLDEN, f), "-L" in e["opts"])
    qname = {(n.decode() if isinstance(n, bytes) else n) if n is not None else "seq%d" % (i + 1): i for i, (n, _) in enumerate(queries)}
    n_checked = 0
    for line in e["out"].splitlines():
        name, st, en, size, cols = pm.parse_line(line)
        q = mm.nt6(queries[qname[name]][1])[st:en]
        occ = pm.occurrences(strings, q)
        assert len(occ) == size
        allowed = set(pm.columns(sorted(occ), en - st, names, lengths))
        assert len(cols) == min(P, size) and len(set(cols)) == len(cols) and set(cols) <= allowed
        if P >= size:
            assert set(cols) == allowed
        n_checked += 1
    assert n_checked == e["lines"]


def test_abi_symbols_and_cli_refusal(tmp_path):
    lib = gpu.load_library()
    for s in ("rb3gpu_ssa_set", "rb3gpu_ssa_keep", "rb3gpu_ssa_drop", "rb3gpu_ssa_info", "rb3gpu_locate", "rb3gpu_mem_pos"):
        assert hasattr(lib, s) and s in gpu.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "rb3gpu.h")).read()
    for s in ("rb3gpu_ssa_set", "rb3gpu_ssa_keep", "rb3gpu_ssa_drop", "rb3gpu_locate", "rb3gpu_mem_pos", "rb3gpu_pos_t", "locate_heap", "locate_slice"):
        assert s in hdr
    # the files are looked for before a device is asked for: the same refusal with and without a GPU
    idx = tmp_path / "k4.fmd"
    idx.write_bytes(open(os.path.join(GOLDEN, "k4_readme.fmd"), "rb").read())
    q = os.path.join(GOLDEN, "mem_iupac.fa")
    msg = b"ERROR: failed to load suffix array samples or sequence names/lengths\n"
    r = subprocess.run([CLI, "mem", "-p", "5", str(idx), q], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == msg
    (tmp_path / "k4.fmd.ssa").write_bytes(b"SSA\2" + bytes(24))
    (tmp_path / "k4.fmd.len.gz").write_bytes(open(os.path.join(GOLDEN, "k4_readme.len.gz"), "rb").read())
    r = subprocess.run([CLI, "mem", "-p", "5", str(idx), q], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == msg
