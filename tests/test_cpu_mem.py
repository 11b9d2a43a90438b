"""mem without a device: what the recorded answers (tests/golden/MEM_MANIFEST.json) must hold, the string model (tests/mem_model.py)
pinned to them on the small indexes, and the host side of the command through librb3host.so and the CLI: the reader that keeps record
names, the line formatter, the --gap and --cov arithmetic, the usage text and the refusals that come before any device work."""
import ctypes
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, host
from tests import mem_model as mm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MEM_MANIFEST.json")))


def test_manifest_condition():
    """at least half of the cases print something; the mutated query on genomes12.fmd prints at least 100 lines at -l19 -c1 and a different,
    non-zero number at -l19 -c2; some case has matches that occur more than once; the regular matrix is whole"""
    assert sum(1 for e in MANIFEST.values() if e["lines"] > 0) * 2 >= len(MANIFEST)
    a = MANIFEST["-l19 -c1 genomes12.fmd mem_mutated.fa.gz"]["lines"]
    b = MANIFEST["-l19 -c2 genomes12.fmd mem_mutated.fa.gz"]["lines"]
    assert a >= 100 and b > 0 and a != b
    assert any(e.get("max_size", 0) > 1 for e in MANIFEST.values())
    idx = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd", "edge_dups.fmd",
           "longruns.fmd", "copies3000.fmd"]
    for i in idx:
        for q in (["mem_mutated.fa.gz"], ["reads_fq.fa.gz"], ["-L", "edge_chars.txt"], ["mem_iupac.fa"]):
            for l in (1, 5, 19, 31, 200):
                for c in (1, 2, 50):
                    key = " ".join(["-l%d" % l, "-c%d" % c] + q[:-1] + [i, q[-1]])
                    assert MANIFEST[key]["matrix"], key
    for i in ("reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"):
        e = MANIFEST["-l19 %s mem_iupac.fa" % i]
        assert e["lines"] == 0 and "both strands" in e["refused"]
    for f in {f for e in MANIFEST.values() for f in e["files"]}:
        assert os.path.exists(os.path.join(GOLDEN, f)), f


def _opt(opts, name, default):
    for o in opts:
        if o.startswith(name) and len(o) > len(name):
            return int(o[len(name):].lstrip("="))
    return default


SMALL = sorted(k for k, e in MANIFEST.items() if e["files"][0] in ("k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd", "edge_dups.fmd")
               and all(f != "reads_fq.fa.gz" and f != "mem_mutated.fa.gz" for f in e["files"]) and "-K" not in e["opts"] and "-K1" not in e["opts"])
_TEXTS = {}


@pytest.mark.parametrize("key", SMALL)
def test_model_matches_recorded(key):
    """the matches found from the strings, by definition, give the reference's bytes on the small indexes (lines, --gap and --cov)"""
    e = MANIFEST[key]
    idx = e["files"][0]
    if idx not in _TEXTS:
        _TEXTS[idx] = mm.Text(mm.index_strings(GOLDEN, idx, CLI))
    is_line = "-L" in e["opts"]
    l, c, gap, cov = _opt(e["opts"], "-l", 19), _opt(e["opts"], "-c", 1), _opt(e["opts"], "--gap", 0), "--cov" in e["opts"]
    out, first = [], 0
    for f in e["files"][1:]:
        qs = mm.read_queries(os.path.join(GOLDEN, f), is_line)
        recs = mm.mem(_TEXTS[idx], [mm.nt6(s) for _, s in qs], l, c)
        names = [n for n, _ in qs]
        if gap > 0 or cov:
            for i, (n, s) in enumerate(qs):
                nm = (n if n is not None else "seq%d" % (first + i + 1)).encode()
                mine = recs[recs["query"] == i]
                if gap > 0:
                    out += [b"%s\t%d\t%d\t%d\n" % (nm, a, b, len(s)) for a, b in mm.gaps(mine, len(s), gap)]
                elif mm.coverage(mine, len(s)) > 0:
                    out.append(b"%s\t%d\t%d\n" % (nm, len(s), mm.coverage(mine, len(s))))
        else:
            out.append(mm.lines(recs, names, first))
        first += len(qs)
    got = b"".join(out)
    assert got.count(b"\n") == e["lines"]
    assert hashlib.md5(got).hexdigest() == e["md5"]


def test_small_cases_are_not_trivial():
    assert len(SMALL) >= 100 and sum(1 for k in SMALL if MANIFEST[k]["lines"] > 0) >= 40


# ---- the host library: reader with names, formatter ----

class _Rec(ctypes.Structure):
    _fields_ = [("query", ctypes.c_int64), ("x0", ctypes.c_int64), ("size", ctypes.c_int64), ("st", ctypes.c_int32), ("en", ctypes.c_int32)]


def _lib():
    L = host.load_library()
    L.rb3h_seq_read1.restype = ctypes.c_int64
    L.rb3h_seq_read1.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_char_p)]
    L.rb3h_seq_error.restype = ctypes.c_int
    L.rb3h_seq_error.argtypes = [ctypes.c_void_p]
    L.rb3h_mem_format.restype = ctypes.c_int
    L.rb3h_mem_format.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    return L


def _read1_all(path, is_line):
    L = _lib()
    fp = L.rb3h_seq_open(str(path).encode(), int(is_line))
    assert fp
    out = []
    seq, name = ctypes.c_void_p(), ctypes.c_char_p()
    while True:
        l = L.rb3h_seq_read1(fp, ctypes.byref(seq), ctypes.byref(name))
        if l < 0:
            break
        out.append((name.value.decode() if name.value is not None else None, ctypes.string_at(seq, l) if l else b""))
    err = L.rb3h_seq_error(fp)
    L.rb3h_seq_close(fp)
    return out, err


@pytest.mark.parametrize("name,is_line", [("mem_mutated.fa.gz", False), ("mem_iupac.fa", False), ("reads_fq.fa.gz", False), ("genomes12_part1.fa.gz", False),
                                          ("edge_chars.txt", True), ("edge_dups.txt", True), ("k4_readme.txt", True)])
def test_reader_keeps_names(name, is_line):
    got, err = _read1_all(os.path.join(GOLDEN, name), is_line)
    want = mm.read_queries(os.path.join(GOLDEN, name), is_line)
    assert err == 0 and got == want and len(got) > 0


def test_reader_grammar(tmp_path):
    """names end at the first white space; empty records and empty lines are records; FASTQ with its quality skipped; several lines per
    record; '\\r' at line ends; a truncated quality string ends the file with an error behind the records before it; gzip or not"""
    p = tmp_path / "a.fa"
    p.write_bytes(b">r1 comment here\nACGT\nacgtn\n>r2\tx\n\n>\n>r3\r\nGG\r\nTT\r\n@q1 c\nACGTA\n+\nIIIII\n@q2\nAC\n+q2\nI\n")
    got, err = _read1_all(p, False)
    assert got == [("r1", b"ACGTacgtn"), ("r2", b""), ("", b""), ("r3", b"GGTT"), ("q1", b"ACGTA")] and err == -2
    g = tmp_path / "a.fa.gz"
    g.write_bytes(gzip.compress(b">only\nAC\nGT\n"))
    assert _read1_all(g, False) == ([("only", b"ACGT")], 0)
    t = tmp_path / "l.txt"
    t.write_bytes(b"ACGT\n\nNNA\r\nTT")
    assert _read1_all(t, True) == ([(None, b"ACGT"), (None, b""), (None, b"NNA"), (None, b"TT")], 0)
    e = tmp_path / "empty.txt"
    e.write_bytes(b"")
    assert _read1_all(e, True) == ([], 0) and _read1_all(e, False) == ([], 0)
    big = tmp_path / "big.txt"      # lines across the reader's buffer boundary (1 MiB), the file a whole number of buffers long
    line = b"ACGTN" * 13107 + b"AC\n"
    assert len(line) == 65538
    big.write_bytes(line * 15 + b"G" * (16 * 65536 - 15 * 65538 - 1) + b"\n")
    got, err = _read1_all(big, True)
    assert os.path.getsize(big) == 1 << 20 and len(got) == 16 and err == 0 and all(s == line[:-1] for _, s in got[:15])


def _format(mode, min_gap, name, qid, length, recs):
    L = _lib()
    arr = (_Rec * max(len(recs), 1))()
    for i, (st, en, size) in enumerate(recs):
        arr[i].query, arr[i].x0, arr[i].size, arr[i].st, arr[i].en = 0, 0, size, st, en
    buf = host._Buf(0, 0, None)
    assert L.rb3h_mem_format(ctypes.byref(buf), mode, min_gap, None if name is None else name.encode(), qid, length, len(recs), arr) == 0
    out = ctypes.string_at(buf.s, buf.l) if buf.l else b""
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    libc.free(buf.s)
    return out


def test_formatter_lines():
    assert _format(0, 0, "chr1", 0, 100, [(0, 30, 1), (31, 71, 10), (40, 100, 123456789012)]) == b"chr1\t0\t30\t1\nchr1\t31\t71\t10\nchr1\t40\t100\t123456789012\n"
    assert _format(0, 0, None, 6, 100, [(5, 2147483647, 0)]) == b"seq7\t5\t2147483647\t0\n"
    assert _format(0, 0, "", 0, 5, [(0, 5, 2)]) == b"\t0\t5\t2\n"
    assert _format(0, 0, "x", 0, 5, []) == b""
    many = [(i, i + 20, i % 7) for i in range(50000)]
    assert _format(0, 0, "n" * 300, 0, 60000, many) == b"".join(b"%s\t%d\t%d\t%d\n" % (b"n" * 300, a, b, c) for a, b, c in many)


def _as_recs(recs):
    r = np.zeros(len(recs), dtype=mm.MEM_REC)
    for i, (st, en, size) in enumerate(recs):
        r[i]["st"], r[i]["en"], r[i]["size"] = st, en, size
    return r


def test_formatter_gap_and_cov_arithmetic():
    """--gap and --cov against the definition (uncovered stretches, covered symbols) on random sets of matches ordered by start whose ends
    grow with their starts, as the matches of a query do"""
    rng = np.random.default_rng(5)
    assert _format(1, 10, "q", 0, 50, []) == b"q\t0\t50\t50\n"
    assert _format(1, 51, "q", 0, 50, []) == b""
    assert _format(2, 0, "q", 0, 50, []) == b""
    assert _format(1, 3, None, 2, 30, [(0, 10, 1), (5, 12, 1), (15, 20, 1), (20, 27, 2)]) == b"seq3\t12\t15\t30\nseq3\t27\t30\t30\n"
    assert _format(2, 0, None, 2, 30, [(0, 10, 1), (5, 12, 1), (15, 20, 1), (20, 27, 2)]) == b"seq3\t30\t24\n"
    for _ in range(300):
        length = int(rng.integers(1, 400))
        n = int(rng.integers(0, 12))
        st = np.sort(rng.choice(length, size=min(n, length), replace=False))
        en, recs = 0, []
        for s in st:
            en = max(en + 1, int(s) + 1 + int(rng.integers(0, 40)))
            en = min(en, length)
            if recs and en <= recs[-1][1]:
                continue
            recs.append((int(s), en, 1))
        min_gap = int(rng.integers(1, 30))
        r = _as_recs(recs)
        want = b"".join(b"q\t%d\t%d\t%d\n" % (a, b, length) for a, b in mm.gaps(r, length, min_gap))
        assert _format(1, min_gap, "q", 0, length, recs) == want
        cov = mm.coverage(r, length)
        assert _format(2, 0, "q", 0, length, recs) == (b"q\t%d\t%d\n" % (length, cov) if cov else b"")


# ---- the CLI before any device work ----

def _cli(args):
    return subprocess.run([CLI, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_cli_usage_and_refusals():
    r = _cli([])
    assert r.returncode == 0 and r.stdout == b"Usage: ropebwt3-amd mem [options] <idx.fmr> <seq.fa> [...]\n"
    assert b"-l INT      min MEM length [19]" in r.stderr and b"--gap=NUM" in r.stderr and b"--cov" in r.stderr and b"-K NUM" in r.stderr
    assert b"-p INT" not in r.stderr and b"--old-mem" not in r.stderr
    assert _cli(["-l25", os.path.join(GOLDEN, "k4_readme.fmd")]).returncode == 0      # (too few arguments: usage)
    files = [os.path.join(GOLDEN, "k4_readme.fmd"), os.path.join(GOLDEN, "mem_iupac.fa")]
    for bad in (["-p", "5"], ["--old-mem"], ["-l0"], ["-l", "-3"], ["-c0"], ["-d"], ["-N", "5"], ["-a", "31"], ["-w9"], ["-e"], ["--all-e2e"], ["--no-ssa"], ["-g", "3"], ["--nonsense"]):
        r = _cli(bad + files)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") >= 1, bad
