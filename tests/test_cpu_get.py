"""get without a device: what the recorded answers (tests/golden/GET_MANIFEST.json) must hold, the LF walk restated on the committed plain BWTs
(tests/walk_model.py) against every recorded answer of an index that has one and against the records the index was built from, the formatter,
and the command before any device work."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from ropebwt3_amd.gpu import get_lines
from tests import kount_model as km
from tests import mem_model as mm
from tests import util
from tests import walk_model as wm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "GET_MANIFEST.json")))
INDEXES = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd", "edge_dups.fmd",
           "longruns.fmd", "copies3000.fmd", "reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"]
WITH_BWT = sorted(k for k, e in MANIFEST.items() if os.path.exists(os.path.join(GOLDEN, os.path.splitext(e["index"])[0] + ".bwt.gz")))
_FM = {}


def _fm(idx):
    if idx not in _FM:
        _FM[idx] = wm.Fm(km.read_plain(os.path.join(GOLDEN, os.path.splitext(idx)[0] + ".bwt.gz")))
    return _FM[idx]


def _records(e):
    """[(row, end row, letters)] of a recorded stdout"""
    ls = e["stdout"].split("\n")
    assert ls[-1] == "" and len(ls) % 2 == 1
    return [(int(ls[i][1:].split()[0]), int(ls[i][1:].split()[1]), ls[i + 1]) for i in range(0, len(ls) - 1, 2)]


def test_manifest_condition():
    """every index has its two regular cases; the large calls are there; the answers the reference gave when the cases were chosen are the recorded
    ones; and some case asks for a row outside the index, some answer is an empty string, some row asked for is not a sentinel's"""
    for i in INDEXES:
        es = [e for e in MANIFEST.values() if e["index"] == i]
        assert any(e["args"][0] == "-1" for e in es) and any(e["rows"][:2] == [0, 1] and e["acc6"] in e["rows"] and e["acc1"] in e["rows"] for e in es), i
    by_rows = {(e["index"], len(e["rows"])): e for e in MANIFEST.values()}
    for idx, n in (("edge_dups.fmd", 14), ("genomes12.fmd", 24), ("reads_fq.fmd", 6104), ("longruns.fmd", 8), ("copies3000.fmd", 100), ("genomes12_first6.fmr", 12)):
        e = by_rows[(idx, n)]
        assert e["rows"] == list(range(n)) and e["lines"] == 2 * n
    assert by_rows[("reads_fq.fmd", 6104)]["acc1"] == 6104 and by_rows[("longruns.fmd", 8)]["acc1"] == 8
    for e in MANIFEST.values():
        assert e["lines"] == 2 * sum(1 for r in e["rows"] if 0 <= r < e["acc6"])         # rows outside print nothing
        assert "stdout" not in e or (hashlib.md5(e["stdout"].encode("latin-1")).hexdigest() == e["md5"] and e["stdout"].count("\n") == e["lines"])
    assert [r[1] for r in _records(by_rows[("edge_dups.fmd", 14)])] == [16, 24, 17, 25, 43, 15, 18, 26, 51, 45, 20, 49, 15, 51]
    e = MANIFEST["-1 k3_both.fmd 0 1 5 99999 abc 7"]
    assert e["rows"] == [0, 1, 5, 99999, 0, 7] and [r[0] for r in _records(e)] == [0, 1, 5, 0, 7]
    assert any(r < 0 or r >= e["acc6"] for e in MANIFEST.values() for r in e["rows"])
    assert any(rec[2] == "" for e in MANIFEST.values() if "stdout" in e for rec in _records(e))
    assert any(e["acc1"] <= r < e["acc6"] for e in MANIFEST.values() for r in e["rows"])
    assert any(len(set(e["rows"])) < len(e["rows"]) for e in MANIFEST.values())           # a row asked for twice


def test_model_covers_enough():
    assert len(WITH_BWT) >= 18 and sum(1 for k in WITH_BWT if "stdout" not in MANIFEST[k]) >= 3


@pytest.mark.parametrize("key", WITH_BWT)
def test_model_matches_recorded(key):
    """the LF walk restated over cumulative counts gives the reference's bytes: line by line where the text is recorded, by md5 otherwise"""
    e = MANIFEST[key]
    got = wm.get_text(_fm(e["index"]), e["rows"])
    if "stdout" in e:
        assert got.decode("latin-1").splitlines() == e["stdout"].splitlines()
    assert got.count(b"\n") == e["lines"] and hashlib.md5(got).hexdigest() == e["md5"]


def test_sentinel_rows_spell_the_records():
    """rows 0 .. acc[1] - 1 of genomes12 are the records of genomes12.fa.gz, both strands interleaved: row 2i forward, row 2i + 1 reverse complement;
    the walk of row k ends at the row of the suffix that IS string k, a row of the first symbol's block or a sentinel's for an empty string"""
    fm = _fm("genomes12.fmd")
    recs = [mm.nt6(s) for _, s in mm.read_queries(os.path.join(GOLDEN, "genomes12.fa.gz"))]
    m = int(fm.acc[1])
    assert m == 2 * len(recs) == 24
    end, seqs = fm.retrieve(np.arange(m))
    for i, s in enumerate(recs):
        assert np.array_equal(seqs[2 * i], s) and np.array_equal(seqs[2 * i + 1], util.revcomp(s)), i
    assert len(set(end.tolist())) == m and all(fm.b[e] == 0 for e in end)
    e2, s2 = fm.retrieve([-1, fm.n, fm.n + 5, m])
    assert e2[:3].tolist() == [-1, -1, -1] and all(s.size == 0 for s in s2[:3]) and e2[3] >= 0 and 0 < s2[3].size < 20001


def test_formatter():
    e = MANIFEST["-1 k3_both.fmd 0 1 5 99999 abc 7"]
    end, seqs = _fm("k3_both.fmd").retrieve(e["rows"])
    assert get_lines(e["rows"], end, seqs).decode() == e["stdout"]
    e = [x for x in MANIFEST.values() if x["index"] == "edge_dups.fmd" and len(x["rows"]) == 14][0]
    end, seqs = _fm("edge_dups.fmd").retrieve(e["rows"])
    assert get_lines(e["rows"], end, seqs).decode() == e["stdout"]
    assert get_lines([], [], []) == b"" and get_lines([9], [-1], [np.zeros(0, dtype=np.uint8)]) == b""
    assert get_lines([3], [2], [np.array([0, 1, 2, 3, 4, 5], dtype=np.uint8)]) == b">3 2\n$ACGTN\n"


# ---- the CLI before any device work ----

def _cli(args):
    return subprocess.run([CLI, "get"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_cli_usage_and_refusals(tmp_path):
    for args in ([], [os.path.join(GOLDEN, "k4_readme.fmd")], ["-1", os.path.join(GOLDEN, "k4_readme.fmd")], [os.path.join(GOLDEN, "k4_readme.fmd"), "-3"]):
        r = _cli(args)
        assert r.returncode == 0 and r.stdout == b"Usage: ropebwt3-amd get <idx.fmr> <int> [...]\n", args
    r = _cli([str(tmp_path / "missing.fmd"), "0"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") >= 1
