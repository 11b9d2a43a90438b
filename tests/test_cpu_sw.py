"""sw -e without a GPU: what tests/golden/SW_MANIFEST.json and the read fixture must hold; the Python model of the alignment
(tests/swaln_model.py: the end_len rule and the full backtrack) against the reference's committed output, line for line; the host
formatters -- the C one of the CLI (swfmt.c, through librb3host.so) and the Python one of ropebwt3_amd.gpu -- on step bytes made by the
model, against the same lines; the refusals that need no device.

Positions: the model does not restate the traversal of the sampled suffix array (tests/test_gpu_sw.py holds the engine's positions
against rb3gpu_locate, whose order tests/test_gpu_mempos.py pins), so on a line with positions the columns 5-9 and the ap / aq tag
are taken from the recorded line, parsed back to (string, offset) pairs, and must come out of the formatters unchanged; every pair
must be an occurrence of the line's rs sequence where the fixture has one.  Everything else on the line is the model's."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, host
from ropebwt3_amd.gpu import POS, SW_ALL_HEADER, sw_all_lines, sw_lines
from tests import kount_model as km
from tests import mem_model as mm
from tests import pos_model as pm
from tests import sw_model as sw
from tests import swaln_model as sa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "SW_MANIFEST.json")))
STDOUT = json.load(open(os.path.join(GOLDEN, "SW_STDOUT.json")))
SYMMETRIC = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
             "edge_dups.fmd", "longruns.fmd", "copies3000.fmd"]
OPT_OF = {"-N": "n_best", "-m": "min_sc", "-A": "match", "-B": "mis", "-O": "gap_open", "-E": "gap_ext", "-y": "e2e_drop"}
G8 = "-s8 %s genomes12.fmd sw_reads.fa"


def _key(e):
    return ("" if e["S"] is None else "-s%d " % e["S"]) + ("nolen " if e["nolen"] else "") + " ".join(e["opts"] + e["files"])


def test_manifest_is_complete():
    for key, e in MANIFEST.items():
        assert key == _key(e) and len(e["md5"]) == 32 and e["lines"] >= 0
        for f in e["files"]:
            assert os.path.exists(os.path.join(GOLDEN, f)), f
        assert (e.get("model", False)) == (key in STDOUT)
        if e["S"] is not None:
            assert os.path.exists(os.path.join(GOLDEN, e["files"][0].split(".")[0] + ".len.gz"))
    for idx in SYMMETRIC:
        for q in ("sw_reads.fa", "mem_iupac.fa", "-L edge_chars.txt"):
            for o in ("-e", "-e -N5", "--all-e2e -b"):
                hit = [e for e in MANIFEST.values() if e["matrix"] and e["files"][0] == idx and " ".join(e["opts"] + e["files"][1:]) == (o + " " + q)]
                assert len(hit) == 1, (idx, q, o)
    for S in (0, 3, 8):
        for p in (1, 3, 50):
            assert MANIFEST["-s%d -e -p%d genomes12.fmd sw_reads.fa" % (S, p)]["lines"] == MANIFEST[G8 % "-e"]["lines"]
    assert len(set(MANIFEST["-s%d -e -p3 genomes12.fmd sw_reads.fa" % S]["md5"] for S in (0, 3, 8))) == 3     # the sample rate decides which positions come first
    for o in ("-e --no-ssa", "-e -k11", "-k5 -e", "-e -k5", "-e -u", "-e --seq", "-e -m10 -y4", "-e -y0", "-e -N1", "-e -N200", "-e -A2 -B4 -O4 -E1", "--all-e2e -g3", "-g1 -b", "-e -K1k"):
        assert MANIFEST[G8 % o]["lines"] > 0, o
    assert MANIFEST[G8 % "-k5 -e"]["md5"] == MANIFEST[G8 % "-e"]["md5"] != MANIFEST[G8 % "-e -k5"]["md5"]   # the order of -e and -k matters
    assert MANIFEST[G8 % "-e -K1k"]["md5"] == MANIFEST[G8 % "-e"]["md5"] == MANIFEST[G8 % "-e -b"]["md5"]   # a batch holds whole queries; -b changes no PAF
    assert MANIFEST[G8 % "-e -u"]["lines"] > MANIFEST[G8 % "-e"]["lines"]
    assert MANIFEST["-s8 nolen -e genomes12.fmd sw_reads.fa"]["md5"] not in (MANIFEST[G8 % "-e"]["md5"], MANIFEST[G8 % "-e --no-ssa"]["md5"])
    assert MANIFEST["-s8 nolen -e -p4 genomes12.fmd mem_iupac.fa"]["refused"] == "ERROR: failed to load suffix array samples or sequence names/lengths"
    assert MANIFEST["-s8 -e genomes12.fmd mem_mutated.fa.gz"]["lines"] > 0
    assert sum(1 for e in MANIFEST.values() if len(e["files"]) > 2) >= 2
    for idx in ("copies3000.fmd", "longruns.fmd"):
        assert MANIFEST["-s8 -e -L -p5 %s sw_runs.txt" % idx]["lines"] > 0
    refused = [e for e in MANIFEST.values() if e["files"][0] in ("reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd")]
    assert len(refused) == 3 and all(e["lines"] == 0 and e["refused"] == "ERROR: BWT doesn't contain both strands" for e in refused)
    model = [e for e in MANIFEST.values() if e.get("model")]
    assert any("-k11" in e["opts"] for e in model) and any("-k5" in e["opts"] for e in model) and any("--all-e2e" in e["opts"] for e in model)
    assert any(e["opts"][0].startswith("-g") for e in model) and any("--seq" in e["opts"] for e in model) and any("sw_reads.fa" in e["files"] for e in model)


def test_fixture_conditions():
    """what the issue asks of sw_reads.fa, on the counts recorded from the reference's output of `sw -e -p3` at -s8"""
    qs = mm.read_queries(os.path.join(GOLDEN, "sw_reads.fa"))
    assert 200 <= len(qs) <= 400 and os.path.getsize(os.path.join(GOLDEN, "sw_reads.fa")) < 64 << 10
    assert sum(1 for _, s in qs if b"N" in s) >= 10 and qs[-1][0] == "random" and max(len(s) for _, s in qs) <= 142
    e = MANIFEST["-s8 -e -p3 genomes12.fmd sw_reads.fa"]
    c = e["counts"]
    assert min(c["I"], c["D"], c["X"], c["minus"], c["ap"]) >= 50, c
    assert c["no_hit"] >= 10 and c["five_plus"] >= 10, c
    assert MANIFEST["-s8 -e -u genomes12.fmd sw_reads.fa"]["lines"] - e["lines"] == c["no_hit"]
    assert MANIFEST["-s8 -e --no-ssa genomes12.fmd sw_reads.fa"]["counts"]["minus"] == 0 == MANIFEST["-s8 -e genomes12.fmd sw_reads.fa"]["counts"]["ap"]


def _model_opts(e):
    o = {}
    f = dict(write_all=False, max_out=0, both=False, unmapped=False, with_rs=False, max_pos=0)
    for x in e["opts"]:
        if x == "-e":
            o["end_len"] = 1
        elif x.startswith("-k"):
            o["end_len"] = int(x[2:])
        elif x == "--all-e2e" or x.startswith("-g"):
            o["end_len"], f["write_all"] = 1, True
            if x.startswith("-g"):
                f["max_out"] = int(x[2:])
        elif x == "-b":
            f["both"] = True
        elif x == "-u":
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
    """the (sid, pos) pairs a recorded PAF line was written from"""
    f = line.split("\t")
    if f[4] == "*":
        return []
    tags = [x for x in f[12:] if x.startswith(("ap:Z:", "aq:Z:"))]
    if names is None:
        out = [(int(f[5]), int(f[7]))]
        out += [tuple(int(v) for v in p.split(",")) for t in tags for p in t[5:].split(";") if p]
        return out
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


def _c_format(lib, name, qid, seq, hits, f, names, lengths, strand="+"):
    """one query through swfmt.c"""
    n = len(hits)
    arr = (_SwHit * max(n, 1))()
    steps, pos = b"", []
    for i, h in enumerate(hits):
        st = bytes(op << 4 | b for op, b in h["steps"])
        ql, rl = sa.lens_of(h["steps"])
        arr[i] = _SwHit(h["lo"], h["hi"], h["score"], ql, rl, len(st), len(steps), len(pos), len(h.get("pos", [])))
        steps += st
        pos += list(h.get("pos", []))
    parr = np.array(pos, dtype=np.int64).reshape(-1, 2)
    out = _Buf(0, 0, None)
    codes = np.ascontiguousarray(seq, dtype=np.uint8)
    sid = None
    if names is not None:
        cn = (ctypes.c_char_p * len(names))(*[x.encode() for x in names])
        cl = (ctypes.c_int64 * len(names))(*lengths)
        sid = _Sid(len(names), cn, cl)
    nm = name.encode() if name is not None else None
    if f["write_all"]:
        r = lib.rb3h_sw_format_all(ctypes.byref(out), nm, qid, len(seq), codes.ctypes.data, n, arr, steps, ctypes.c_char(strand.encode()), f["max_out"])
    else:
        r = lib.rb3h_sw_format_paf(ctypes.byref(out), nm, qid, len(seq), codes.ctypes.data, n, arr, steps, parr.ctypes.data if len(pos) else None,
                                   ctypes.byref(sid) if sid else None, int(f["unmapped"]), int(f["with_rs"]))
    assert r == 0
    got = ctypes.string_at(out.s, out.l) if out.l else b""
    ctypes.CDLL(None).free(ctypes.c_void_p(out.s))
    return got


def _host_lib():
    lib = host.load_library()
    for fn in ("rb3h_sw_format_paf", "rb3h_sw_format_all"):
        getattr(lib, fn).restype = ctypes.c_int
    lib.rb3h_sw_format_paf.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.rb3h_sw_format_all.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p,
                                       ctypes.c_char, ctypes.c_int64]
    return lib


@pytest.mark.parametrize("key", sorted(STDOUT))
def test_model_and_formatters_reproduce_reference(key):
    """every committed case: the model's hits, written by the model's own formatter, by swfmt.c and by ropebwt3_amd.gpu, are the reference's lines"""
    e = MANIFEST[key]
    o, f = _model_opts(e)
    ix = _index(e["files"][0])
    lib = _host_lib()
    names = lengths = None
    if e["S"] is not None and not e["nolen"] and "--no-ssa" not in e["opts"] and not f["write_all"]:
        names, lengths = pm.read_len_gz(os.path.join(GOLDEN, e["files"][0].split(".")[0] + ".len.gz"))
    want = STDOUT[key].splitlines(True)
    at = len(sa.ALL_HEADER.splitlines()) if f["write_all"] else 0
    if f["write_all"]:
        assert "".join(want[:at]).encode() == sa.ALL_HEADER == SW_ALL_HEADER
    qid = 0
    strings = None
    for fn in e["files"][1:]:
        for name, s in mm.read_queries(os.path.join(GOLDEN, fn), "-L" in e["opts"]):
            q = mm.nt6(s)
            hits = sa.align(ix, q, o)
            if f["write_all"]:
                blocks = [("+", q, hits)]
                if f["both"]:
                    r = sa.revcomp6(q)
                    blocks.append(("-", r, sa.align(ix, r, o)))
                for strand, codes, hs in blocks:
                    mine = sa.all_hits_block(name, qid, codes, hs, strand, f["max_out"])
                    n = mine.count(b"\n")
                    assert mine.decode() == "".join(want[at:at + n]), (name, qid, strand)
                    assert _c_format(lib, name, qid, codes, hs, f, None, None, strand) == mine
                    at += n
                api = [[dict(lo=h["lo"], hi=h["hi"], score=h["score"], steps=bytes(op << 4 | b for op, b in h["steps"])) for h in hs] for _, _, hs in blocks]
                both = sw_all_lines([q], [api[0]], [name], first_id=qid, max_out=f["max_out"], hits_rev=[api[1]] if f["both"] else None)
                assert both.decode() == "".join(want[at - both.count(b"\n"):at])
            else:
                n = len(hits) if hits else int(f["unmapped"])
                lines = want[at:at + n]
                for h, line in zip(hits, lines):
                    rlen = sa.lens_of(h["steps"])[1]
                    h["pos"] = _positions_of(line.rstrip("\n"), names, lengths, rlen)
                    if h["pos"] and f["with_rs"] and names is not None:     # a recorded position is an occurrence of the aligned sequence
                        if strings is None:
                            strings = km.strings_of(km.golden_plain(GOLDEN, e["files"][0], _build.BIN_CLI))
                        rs = bytes(b for op, b in h["steps"] if op != sa.OP_I)
                        for sid, p in h["pos"]:
                            assert pm.as_bytes(strings[sid])[p:p + rlen] == rs
                if e["S"] is not None and "--no-ssa" not in e["opts"]:
                    assert [len(h["pos"]) for h in hits] == sa.n_positions(hits, f["max_pos"])
                mine = b"".join(sa.paf_line(name, qid, q, h, h["pos"], names, lengths, f["with_rs"]) for h in hits) if hits else (sa.unmapped_line(name, qid, q) if f["unmapped"] else b"")
                assert mine.decode() == "".join(lines), (name, qid)
                assert _c_format(lib, name, qid, q, hits, f, names, lengths) == mine
                api = [dict(lo=h["lo"], hi=h["hi"], score=h["score"], qlen=len(q), rlen=sa.lens_of(h["steps"])[1], steps=bytes(op << 4 | b for op, b in h["steps"]),
                            pos=np.array(h["pos"], dtype=np.int64).reshape(-1, 2).view(POS).reshape(-1)) for h in hits]
                assert sw_lines([q], [api], [name], first_id=qid, seq_names=names, lengths=lengths, unmapped=f["unmapped"], with_rs=f["with_rs"]) == mine
                at += n
            qid += 1
    assert at == len(want)


def test_end_len_rule():
    """the query is consumed from its end: a mismatch 8 symbols from the end is met in row 8, where 7 symbols are aligned -- allowed at end_len 1
    (and the score, 7 - 3, stays positive), not at end_len 11, where the read then has no end-to-end alignment at all"""
    ix = _index("genomes12.fmd")
    g = next(s for _, s in mm.read_queries(os.path.join(GOLDEN, "genomes12.fa.gz")))
    read = bytearray(g[1000:1060].upper())
    read[-8] = ord("A") if read[-8] != ord("A") else ord("C")
    q = mm.nt6(bytes(read))
    a = sa.align(ix, q, dict(end_len=1))
    assert a and sa.cigar_of(a[0]["steps"])[0] == [(52, sa.OP_EQ), (1, sa.OP_X), (7, sa.OP_EQ)] and a[0]["score"] == 59 - 3
    assert sa.align(ix, q, dict(end_len=7)) == a and sa.align(ix, q, dict(end_len=8)) == [] == sa.align(ix, q, dict(end_len=11))
    assert sa.n_positions([dict(lo=0, hi=5), dict(lo=0, hi=1), dict(lo=0, hi=9)], 6) == [5, 1, 1]      # the budget is used up: one position from then on
    assert sa.n_positions([dict(lo=0, hi=5), dict(lo=0, hi=9)], 0) == [1, 1]


def test_cli_refusals_without_a_device(tmp_path):
    """what `sw` refuses before it asks for a device: one line on stderr, nothing on stdout, exit 1"""
    cli = _build.BIN_CLI
    idx, q = os.path.join(GOLDEN, "genomes12.fmd"), os.path.join(GOLDEN, "mem_iupac.fa")
    for bad in ([], ["-k5"], ["-e", "-j2"], ["-e", "-k5", "-j6"], ["-e", "-N0"], ["-e", "-k0"], ["-e", "-a5"], ["-e", "-w5"], ["-e", "-l5"], ["-e", "-c2"], ["-e", "-d"],
                ["-e", "--gap=20"], ["-e", "--cov"], ["-e", "--old-mem"]):
        r = subprocess.run([cli, "sw"] + bad + [idx, q], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1, bad
    r = subprocess.run([cli, "sw", idx, q], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"local mode is not implemented: use -e" in r.stderr
    u = subprocess.run([cli], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"    sw  " in u.stdout + u.stderr
    u = subprocess.run([cli, "sw"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert u.returncode == 0 and b"Usage: ropebwt3-amd sw" in u.stdout and b"--all-e2e" in u.stderr
