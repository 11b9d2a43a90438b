"""suffix without a device: what the recorded answers (tests/golden/SUFFIX_MANIFEST.json) must hold, the walk restated on the committed plain
BWTs (tests/walk_model.py) against every recorded answer of an index that has one, the formatter, and the command before any device work."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from ropebwt3_amd.gpu import SUFFIX_OUT, suffix_lines
from tests import kount_model as km
from tests import mem_model as mm
from tests import walk_model as wm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "SUFFIX_MANIFEST.json")))
INDEXES = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd", "edge_dups.fmd",
           "longruns.fmd", "copies3000.fmd", "reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"]
WITH_BWT = sorted(k for k, e in MANIFEST.items() if os.path.exists(os.path.join(GOLDEN, os.path.splitext(e["files"][0])[0] + ".bwt.gz")))
_FM = {}


def _fm(idx):
    if idx not in _FM:
        _FM[idx] = wm.Fm(km.read_plain(os.path.join(GOLDEN, os.path.splitext(idx)[0] + ".bwt.gz")))
    return _FM[idx]


def _cols(e):
    return [l.split("\t") for l in e["stdout"].splitlines()]


def test_manifest_condition():
    """the regular matrix is whole, the two cases outside it are there, the answers the reference gave when the cases were chosen are the recorded
    ones, and all four kinds of line occur: the whole query found, a proper suffix found, nothing found, a query of no symbols"""
    for i in INDEXES:
        for q in (["mem_mutated.fa.gz"], ["reads_fq.fa.gz"], ["-L", "edge_chars.txt"], ["mem_iupac.fa"], ["sw_reads.fa"]):
            assert MANIFEST[" ".join(q[:-1] + [i, q[-1]])]["matrix"]
    assert len(MANIFEST) == len(INDEXES) * 5 + 2
    for e in MANIFEST.values():
        assert e["lines"] > 0 and all(os.path.exists(os.path.join(GOLDEN, f)) for f in e["files"])
        assert "stdout" not in e or (hashlib.md5(e["stdout"].encode("latin-1")).hexdigest() == e["md5"] and e["stdout"].count("\n") == e["lines"])
    assert _cols(MANIFEST["genomes12.fmd mem_iupac.fa"])[:5] == [["iupac", "400", "400", "0"], ["empty", "0", "0", "0"], ["short", "0", "12", "10"],
                                                                 ["nocomment", "0", "160", "1"], ["allN", "25", "25", "0"]]
    assert _cols(MANIFEST["genomes12.fmd mem_mutated.fa.gz"]) == [["seq0_mut1", "19846", "20002", "1"], ["seq1_mut2", "19946", "19998", "11"]]
    whole = _cols(MANIFEST["genomes12.fmd genomes12_part1.fa.gz"])
    assert len(whole) >= 2 and all(c[1] == "0" and int(c[2]) >= 20000 and int(c[3]) >= 1 for c in whole)
    multi = _cols(MANIFEST["-L genomes12.fmd edge_chars.txt edge_dups.txt edge_chars.txt"])
    assert [c[0] for c in multi] == ["seq%d" % (i + 1) for i in range(len(multi))]      # the running record number, over the files
    kinds = set()
    for e in MANIFEST.values():
        for c in (_cols(e) if "stdout" in e else []):
            start, length, size = int(c[1]), int(c[2]), int(c[3])
            kinds.add("empty" if length == 0 else "whole" if start == 0 else "none" if start == length else "proper")
            assert (size == 0) == (start == length) and 0 <= start <= length
    assert kinds == {"empty", "whole", "none", "proper"}


def test_model_covers_enough():
    assert len(WITH_BWT) >= 40 and sum(1 for k in WITH_BWT if "stdout" not in MANIFEST[k]) >= 5


@pytest.mark.parametrize("key", WITH_BWT)
def test_model_matches_recorded(key):
    """the walk restated over cumulative counts gives the reference's bytes: line by line where the text is recorded, by md5 otherwise"""
    e = MANIFEST[key]
    got = wm.suffix_text(_fm(e["files"][0]), [os.path.join(GOLDEN, f) for f in e["files"][1:]], "-L" in e["opts"])
    if "stdout" in e:
        assert got.decode("latin-1").splitlines() == e["stdout"].splitlines()
    assert got.count(b"\n") == e["lines"] and hashlib.md5(got).hexdigest() == e["md5"]


def test_reads_of_the_index_are_found_whole():
    """every record of reads_fq.fa.gz is in reads_fq.fmd: start 0 on all 3052"""
    qs = mm.read_queries(os.path.join(GOLDEN, "reads_fq.fa.gz"))
    start, length, size = _fm("reads_fq.fmd").suffix([mm.nt6(s) for _, s in qs])
    assert len(qs) == 3052 and not start.any() and (size >= 1).all() and (length > 0).all()


def test_formatter():
    e = MANIFEST["genomes12.fmd mem_iupac.fa"]
    qs = mm.read_queries(os.path.join(GOLDEN, "mem_iupac.fa"))
    start, length, size = _fm("genomes12.fmd").suffix([mm.nt6(s) for _, s in qs])
    r = np.zeros(len(qs), dtype=SUFFIX_OUT)
    r["query"], r["start"], r["length"], r["size"] = np.arange(len(qs)), start, length, size
    assert suffix_lines(r, [n for n, _ in qs]).decode() == e["stdout"]
    e = MANIFEST["-L genomes12.fmd edge_chars.txt edge_dups.txt edge_chars.txt"]
    got, first = b"", 0
    for f in e["files"][1:]:
        qs = mm.read_queries(os.path.join(GOLDEN, f), True)
        start, length, size = _fm("genomes12.fmd").suffix([mm.nt6(s) for _, s in qs])
        r = np.zeros(len(qs), dtype=SUFFIX_OUT)
        r["query"], r["start"], r["length"], r["size"] = np.arange(len(qs)), start, length, size
        got += suffix_lines(r, None, first_id=first)
        first += len(qs)
    assert got.decode("latin-1") == e["stdout"]
    assert suffix_lines(r[:1], [None], first_id=6).startswith(b"seq7\t") and suffix_lines(r[:1], ["x"]).startswith(b"x\t") and suffix_lines(r[:0]) == b""


# ---- the CLI before any device work ----

def _cli(args):
    return subprocess.run([CLI, "suffix"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_cli_usage_and_refusals(tmp_path):
    for args in ([], ["-L"], [os.path.join(GOLDEN, "k4_readme.fmd")], ["-L", os.path.join(GOLDEN, "k4_readme.fmd")]):
        r = _cli(args)
        assert r.returncode == 0 and r.stdout == b"Usage: ropebwt3-amd suffix [options] <idx.fmr> <seq.fa> [...]\n", args
        assert b"  -L        one sequence per line in the input\n" in r.stderr
    r = _cli([str(tmp_path / "missing.fmd"), os.path.join(GOLDEN, "mem_iupac.fa")])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") >= 1
    top = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"    suffix " in top.stdout and b"    get " in top.stdout
