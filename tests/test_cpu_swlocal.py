"""sw --local without a GPU: the host's DAWG builder (dawg.c) against the model's; the Python model of the local alignment
(tests/swlocal_model.py: the DAWG, the general row loop and the backtrack) against the reference's committed output, line for line, with
the host formatters -- swfmt.c through librb3host.so and ropebwt3_amd.gpu.sw_lines -- on step bytes made by the model; what
tests/golden/SWLOCAL_MANIFEST.json must hold; the refusals that need no device.

Positions are taken from the recorded line as in tests/test_cpu_sw.py: the model does not restate the traversal of the sampled suffix array."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, host
from ropebwt3_amd.gpu import POS, sw_lines
from tests import kount_model as km
from tests import mem_model as mm
from tests import pos_model as pm
from tests import sw_model as sw
from tests import swaln_model as sa
from tests import swlocal_model as sl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "SWLOCAL_MANIFEST.json")))
STDOUT = json.load(open(os.path.join(GOLDEN, "SWLOCAL_STDOUT.json")))
SYMMETRIC = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
             "edge_dups.fmd", "longruns.fmd", "copies3000.fmd"]
OPT_OF = {"-N": "n_best", "-m": "min_sc", "-A": "match", "-B": "mis", "-O": "gap_open", "-E": "gap_ext", "-k": "end_len"}
G8 = "-s8 %sgenomes12.fmd sw_reads.fa"
CUT = {}     # case -> (nodes where max_min_sc was above 0, nodes), filled by the model test


def _key(e):
    return ("" if e["S"] is None else "-s%d " % e["S"]) + ("nolen " if e["nolen"] else "") + " ".join(e["opts"] + e["files"])


def _same_dawg(seq):
    g = sl.dawg(seq)
    d = host.dawg(seq)
    assert d["node_off"].tolist() == [0, g.n_node] and d["sym"].tolist() == g.sym
    assert d["qoff0"].tolist() == g.qoff0 and d["n_qoff"].tolist() == g.n_qoff
    assert [d["pre"][d["pre_off"][i]:d["pre_off"][i + 1]].tolist() for i in range(g.n_node)] == g.pre
    return g


def test_dawg_builder_matches_model():
    deg = 0
    for fn, is_line in (("sw_reads.fa", False), ("mem_iupac.fa", False), ("sw_runs.txt", True)):
        for _, s in mm.read_queries(os.path.join(GOLDEN, fn), is_line):
            g = _same_dawg(mm.nt6(s))
            deg = max(deg, max(len(p) for p in g.pre))
    assert deg > 4                                            # an in-degree is not bounded by the alphabet
    g = _same_dawg([])
    assert g.n_node == 1 and g.pre == [[]] and g.qoff0 == [0] and g.n_qoff == [1]
    g = _same_dawg([3])
    assert g.n_node == 2 and g.sym == [0, 3] and g.pre == [[], [0]] and g.qoff0 == [1, 0]
    g = _same_dawg([2] * 9)                                   # a homopolymer: a chain, node i the run of i symbols, which starts in 10 - i places
    assert g.n_node == 10 and g.pre == [[]] + [[i] for i in range(9)] and g.n_qoff == [10 - i for i in range(10)]
    g = _same_dawg([1, 2, 1, 2, 1, 2, 1, 2])
    assert max(g.n_qoff[1:]) == 4
    g = _same_dawg([5] * 6)                                   # N counts as A
    assert g.sym == [0] + [1] * 6
    g = _same_dawg(mm.nt6(b"CAAAAAAT"))
    assert max(len(p) for p in g.pre) == 7                    # CA, CAA, ... all begin at the one C: one node, reached from the seven runs of A
    # a batch is the graphs one after another
    qs = [mm.nt6(s) for _, s in mm.read_queries(os.path.join(GOLDEN, "mem_iupac.fa"))] + [np.zeros(0, dtype=np.uint8)]
    off = np.concatenate([[0], np.cumsum([len(q) for q in qs])])
    b = host.dawg_batch(off, np.concatenate(qs))
    for i, q in enumerate(qs):
        one = host.dawg(q)
        lo, hi = int(b["node_off"][i]), int(b["node_off"][i + 1])
        assert hi - lo == one["sym"].size and np.array_equal(b["sym"][lo:hi], one["sym"]) and np.array_equal(b["qoff0"][lo:hi], one["qoff0"])
        assert np.array_equal(b["pre_off"][lo:hi + 1] - b["pre_off"][lo], one["pre_off"])
        assert np.array_equal(b["pre"][b["pre_off"][lo]:b["pre_off"][hi]], one["pre"])


def test_manifest_is_complete():
    for key, e in MANIFEST.items():
        assert key == _key(e) and len(e["md5"]) == 32 and e["lines"] >= 0
        for f in e["files"]:
            assert os.path.exists(os.path.join(GOLDEN, f)), f
        assert (e.get("model", False)) == (key in STDOUT)
        assert "--local" not in e["opts"] and "-e" not in e["opts"]       # the reference's own options: its default mode
    for idx in SYMMETRIC:
        for q in ("sw_reads.fa", "mem_iupac.fa", "-L edge_chars.txt"):
            for o in ("", "-k5", "-N5", "-m10 -k3"):
                hit = [e for e in MANIFEST.values() if e["matrix"] and e["files"][0] == idx and " ".join(e["opts"] + e["files"][1:]) == (o + " " + q).strip()]
                assert len(hit) == 1, (idx, q, o)
    assert [MANIFEST[G8 % o]["lines"] for o in ("", "-k5 ", "-N5 ", "-m10 -k3 ")] == [216, 217, 213, 241]
    c = MANIFEST[G8 % ""]["counts"]
    assert min(c["I"], c["D"], c["X"]) >= 20 and c["minus"] >= 50, c
    for S in (0, 3, 8):
        for p in (1, 3, 50):
            assert MANIFEST["-s%d -p%d genomes12.fmd sw_reads.fa" % (S, p)]["lines"] == 216
        assert MANIFEST["-s%d -p3 genomes12.fmd sw_reads.fa" % S]["counts"]["ap"] > 0
    assert len(set(MANIFEST["-s%d -p3 genomes12.fmd sw_reads.fa" % S]["md5"] for S in (0, 3, 8))) == 3
    assert MANIFEST[G8 % "-u "]["lines"] > 216 and MANIFEST[G8 % "-u "]["counts"]["unmapped"] == MANIFEST[G8 % "-u "]["lines"] - 216
    for o in ("--no-ssa ", "--seq ", "-N1 ", "-N200 ", "-A2 -B4 -O4 -E1 ", "-K1k ", "-j5 "):
        assert MANIFEST[G8 % o]["lines"] > 0, o
    assert MANIFEST[G8 % "-K1k "]["md5"] == MANIFEST[G8 % ""]["md5"] == MANIFEST[G8 % "-t3 -C 1k -M -b -y3 "]["md5"] == MANIFEST[G8 % "-j5 "]["md5"]
    assert MANIFEST[G8 % "--no-ssa "]["counts"]["minus"] == 0
    assert MANIFEST["-s8 nolen genomes12.fmd sw_reads.fa"]["md5"] not in (MANIFEST[G8 % ""]["md5"], MANIFEST[G8 % "--no-ssa "]["md5"])
    assert MANIFEST["-s8 nolen -p4 genomes12.fmd mem_iupac.fa"]["refused"] == "ERROR: failed to load suffix array samples or sequence names/lengths"
    assert MANIFEST["-s8 -m10 -k3 genomes12.fmd mem_iupac.fa"]["lines"] == 5
    assert "*ng" in STDOUT["-s8 -m10 -k3 genomes12.fmd mem_iupac.fa"] and "*nc" in STDOUT["-s8 -m10 -k3 genomes12.fmd mem_iupac.fa"]
    for idx in ("copies3000.fmd", "genomes12.fmd"):
        e = MANIFEST["-s8 -L -m5 -k2 %s sw_runs.txt" % idx]
        assert e["lines"] == 12 and e["counts"]["qh"] == 9
    assert MANIFEST["-s8 -L -m5 -k2 longruns.fmd sw_runs.txt"]["counts"]["rh_max"] > 900000      # intervals of a million rows
    assert MANIFEST["reads_fq.fmd reads_fq.fa.gz"]["lines"] == 3052 and MANIFEST["-s8 -m10 -k3 genomes12.fmd reads_fq.fa.gz"]["lines"] == 3020
    assert MANIFEST["-s8 genomes12.fmd mem_mutated.fa.gz"]["lines"] > 0
    assert sum(1 for e in MANIFEST.values() if len(e["files"]) > 2) >= 2
    refused = [e for e in MANIFEST.values() if e["files"][0] in ("reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd")]
    assert len(refused) == 3 and all(e["lines"] == 0 and e["refused"] == "ERROR: BWT doesn't contain both strands" for e in refused)
    model = [e for e in MANIFEST.values() if e.get("model")]
    assert any("-u" in e["opts"] for e in model) and any("--seq" in e["opts"] for e in model) and any("sw_reads.fa" in e["files"] for e in model)
    assert any(e["counts"]["qh"] > 0 for e in model) and any(e["counts"]["ap"] > 0 for e in model)
    assert any(min(e["counts"]["I"], e["counts"]["D"], e["counts"]["X"]) > 0 for e in model)


def _model_opts(e):
    o = {}
    f = dict(unmapped=False, with_rs=False, max_pos=0)
    for x in e["opts"]:
        if x == "-u":
            f["unmapped"] = True
        elif x == "--seq":
            f["with_rs"] = True
        elif x.startswith("-p"):
            f["max_pos"] = int(x[2:])
        elif x[:2] in OPT_OF:
            o[OPT_OF[x[:2]]] = int(x[2:])
    return o, f


_INDEXES = {}


def _index(name):
    if name not in _INDEXES:
        _INDEXES[name] = sw.BwtIndex(km.golden_plain(GOLDEN, name, _build.BIN_CLI))
    return _INDEXES[name]


def _positions_of(line, names, lengths, rlen):
    """the (sid, pos) pairs a recorded PAF line was written from (as tests/test_cpu_sw.py)"""
    f = line.split("\t")
    if f[4] == "*":
        return []
    tags = [x for x in f[12:] if x.startswith(("ap:Z:", "aq:Z:"))]
    if names is None:
        return [(int(f[5]), int(f[7]))] + [tuple(int(v) for v in p.split(",")) for t in tags for p in t[5:].split(";") if p]
    where = {n: i for i, n in enumerate(names)}

    def back(name, strand, st):
        s, clen = where[name], lengths[where[name]]
        return (2 * s, st) if strand == "+" else (2 * s + 1, clen - st - rlen)
    out = [back(f[5], f[4], int(f[7]))]
    for t in tags:
        for p in t[5:].split(";"):
            if p:
                name, strand, st = p.rsplit(",", 2)
                out.append(back(name, strand, int(st)))
    return out


class _SwHit(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_int64), ("hi", ctypes.c_int64), ("score", ctypes.c_int32), ("qlen", ctypes.c_int32), ("rlen", ctypes.c_int32), ("n_steps", ctypes.c_int32),
                ("step_off", ctypes.c_int64), ("pos_off", ctypes.c_int64), ("n_pos", ctypes.c_int64)]


class _Buf(ctypes.Structure):
    _fields_ = [("l", ctypes.c_int64), ("m", ctypes.c_int64), ("s", ctypes.c_void_p)]


class _Sid(ctypes.Structure):
    _fields_ = [("n_seq", ctypes.c_int64), ("name", ctypes.POINTER(ctypes.c_char_p)), ("len", ctypes.POINTER(ctypes.c_int64))]


def _host_lib():
    lib = host.load_library()
    lib.rb3h_sw_format_paf_at.restype = ctypes.c_int
    lib.rb3h_sw_format_paf_at.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _c_format(lib, name, qid, seq, hit, f, names, lengths):
    """one query through swfmt.c"""
    arr = (_SwHit * 1)()
    steps, pos = b"", []
    if hit is not None:
        steps = bytes(op << 4 | b for op, b in hit["steps"])
        ql, rl = sa.lens_of(hit["steps"])
        pos = list(hit.get("pos", []))
        arr[0] = _SwHit(hit["lo"], hit["hi"], hit["score"], ql, rl, len(steps), 0, 0, len(pos))
    parr = np.array(pos, dtype=np.int64).reshape(-1, 2)
    out = _Buf(0, 0, None)
    codes = np.ascontiguousarray(seq, dtype=np.uint8)
    sid = None
    if names is not None:
        cn = (ctypes.c_char_p * len(names))(*[x.encode() for x in names])
        cl = (ctypes.c_int64 * len(names))(*lengths)
        sid = _Sid(len(names), cn, cl)
    q0 = np.array([hit["qoff0"] if hit else 0], dtype=np.int32)
    nq = np.array([hit["n_qoff"] if hit else 0], dtype=np.int32)
    r = lib.rb3h_sw_format_paf_at(ctypes.byref(out), name.encode() if name is not None else None, qid, len(seq), codes.ctypes.data, 0 if hit is None else 1, arr, steps,
                                  parr.ctypes.data if len(pos) else None, ctypes.byref(sid) if sid else None, int(f["unmapped"]), int(f["with_rs"]), q0.ctypes.data, nq.ctypes.data)
    assert r == 0
    got = ctypes.string_at(out.s, out.l) if out.l else b""
    ctypes.CDLL(None).free(ctypes.c_void_p(out.s))
    return got


@pytest.mark.parametrize("key", sorted(STDOUT))
def test_model_and_formatters_reproduce_reference(key):
    """every committed case: the model's hit, written by the model's own formatter, by swfmt.c and by ropebwt3_amd.gpu, is the reference's line"""
    e = MANIFEST[key]
    o, f = _model_opts(e)
    ix = _index(e["files"][0])
    lib = _host_lib()
    names = lengths = None
    if e["S"] is not None and not e["nolen"] and "--no-ssa" not in e["opts"]:
        names, lengths = pm.read_len_gz(os.path.join(GOLDEN, e["files"][0].split(".")[0] + ".len.gz"))
    want = STDOUT[key].splitlines(True)
    at = qid = n_cut = n_node = 0
    for fn in e["files"][1:]:
        for name, s in mm.read_queries(os.path.join(GOLDEN, fn), "-L" in e["opts"]):
            q = mm.nt6(s)
            h = sl.align(ix, q, o)
            n_cut, n_node = n_cut + sl.align.last["n_cut"], n_node + sl.align.last["n_node"]
            n = 1 if h is not None else int(f["unmapped"])
            lines = want[at:at + n]
            if h is not None:
                rlen = sa.lens_of(h["steps"])[1]
                h["pos"] = _positions_of(lines[0].rstrip("\n"), names, lengths, rlen)
                if e["S"] is not None and "--no-ssa" not in e["opts"]:
                    assert len(h["pos"]) == sl.n_positions(h, f["max_pos"])
                mine = sl.paf_line(name, qid, q, h, h["pos"], names, lengths, f["with_rs"])
            else:
                mine = sl.unmapped_line(name, qid, q) if f["unmapped"] else b""
            assert mine.decode() == "".join(lines), (name, qid)
            assert _c_format(lib, name, qid, q, h, f, names, lengths) == mine
            api = [] if h is None else [dict(lo=h["lo"], hi=h["hi"], score=h["score"], qlen=sa.lens_of(h["steps"])[0], rlen=sa.lens_of(h["steps"])[1],
                                             steps=bytes(op << 4 | b for op, b in h["steps"]), qoff0=h["qoff0"], n_qoff=h["n_qoff"],
                                             pos=np.array(h["pos"], dtype=np.int64).reshape(-1, 2).view(POS).reshape(-1))]
            assert sw_lines([q], [api], [name], first_id=qid, seq_names=names, lengths=lengths, unmapped=f["unmapped"], with_rs=f["with_rs"]) == mine
            at += n
            qid += 1
    assert at == len(want)
    CUT[key] = (n_cut, n_node)
    if key == G8 % "":       # the cut of a node with several predecessors bites on the read fixture: 15 of its 31233 nodes at the defaults
        assert n_cut == 15 and n_node == 31233, (n_cut, n_node)
    if key == G8 % "-A2 -B4 -O4 -E1 ":
        assert n_cut > 1000, n_cut


def test_n_counts_as_a():
    """an N of the query sits on a node of symbol 1: against an indexed A it scores a match and prints `=`, against G the cs string names the real symbol"""
    text = STDOUT["-s8 -m10 -k3 genomes12.fmd mem_iupac.fa"]
    assert "*ng" in text and "*nc" in text
    ix = _index("genomes12.fmd")
    g = next(s for _, s in mm.read_queries(os.path.join(GOLDEN, "genomes12.fa.gz")))
    at = next(i for i in range(1000, 2000) if g[i:i + 1].upper() == b"A")
    read = bytearray(g[at - 20:at + 20].upper())
    read[20] = ord("N")
    h = sl.align(ix, mm.nt6(bytes(read)), dict(min_sc=30))
    assert h is not None and h["score"] == 40 and sa.cigar_of(h["steps"])[0] == [(40, sa.OP_EQ)] and h["qoff0"] == 0


def test_cli_refusals_without_a_device():
    """what `sw --local` refuses before it asks for a device: one line on stderr, nothing on stdout, exit 1"""
    cli = _build.BIN_CLI
    idx, q = os.path.join(GOLDEN, "genomes12.fmd"), os.path.join(GOLDEN, "mem_iupac.fa")
    for bad in (["--local", "-e"], ["-e", "--local"], ["--local", "--all-e2e"], ["--local", "-g3"], ["--local", "-j12"], ["--local", "-k5", "-j6"], ["--local", "-N0"],
                ["--local", "-k0"], ["--local", "-a5"], ["--local", "-w5"], ["--local", "-l5"], ["--local", "-c2"], ["--local", "-d"], ["--local", "--gap=20"],
                ["--local", "--cov"], ["--local", "--old-mem"]):
        r = subprocess.run([cli, "sw"] + bad + [idx, q], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1, bad
    u = subprocess.run([cli, "sw"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert u.returncode == 0 and b"--local" in u.stderr


def test_abi_symbols():
    lib = ctypes.CDLL(_build.LIB_GPU)
    assert hasattr(lib, "rb3gpu_sw_local") and hasattr(lib, "rb3gpu_sw_e2e")
    hl = host.load_library()
    for fn in ("rb3h_dawg_build", "rb3h_dawg_batch", "rb3h_dawg_free", "rb3h_sw_format_paf_at", "rb3h_sw_format_paf"):
        assert hasattr(hl, fn), fn
