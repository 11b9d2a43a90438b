"""get in pieces without a device: the model of the piece path (tests/piece_model.py) against every recorded answer of an index that has a committed
plain BWT, at three splitter spacings; one example worked by hand; and what the command refuses before any device work."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import kount_model as km
from tests import piece_model as pm
from tests import walk_model as wm

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "GET_MANIFEST.json")))
WITH_BWT = sorted(k for k, e in MANIFEST.items() if os.path.exists(os.path.join(GOLDEN, os.path.splitext(e["index"])[0] + ".bwt.gz")))
_FM, _PC = {}, {}


def _pieces(idx, S):
    if idx not in _FM:
        _FM[idx] = wm.Fm(km.read_plain(os.path.join(GOLDEN, os.path.splitext(idx)[0] + ".bwt.gz")))
    if (idx, S) not in _PC:
        _PC[(idx, S)] = pm.Pieces(_FM[idx], S)
    return _PC[(idx, S)]


def test_model_covers_enough():
    assert len(WITH_BWT) >= 18 and sum(1 for k in WITH_BWT if "stdout" not in MANIFEST[k]) >= 3


@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("key", WITH_BWT)
def test_model_matches_recorded(key, S):
    """the piece path restated gives the reference's bytes: line by line where the text is recorded, by md5 otherwise"""
    e = MANIFEST[key]
    pc = _pieces(e["index"], S)
    got = pm.get_text(pc, e["rows"])
    if "stdout" in e:
        assert got.decode("latin-1").splitlines() == e["stdout"].splitlines()
    assert got.count(b"\n") == e["lines"] and hashlib.md5(got).hexdigest() == e["md5"]
    m, n = e["acc1"], e["acc6"]
    st = pc.retrieve(e["rows"])[2]
    assert st["n_pieces"] == m + -(-(n - m) // (1 << S)) and pc.steps.sum() == n      # every row of the index is on exactly one piece
    end, seqs = pc.fm.retrieve(e["rows"])
    assert st["n_symbols"] == sum(s.size for s in seqs)


def test_worked_example():
    """Two strings, AC and GA, at S = 1.  The suffixes in order and the symbol in front of each:
        row 0  $0       C        row 3  AC$0   $
        row 1  $1       A        row 4  C$0    A
        row 2  A$1      G        row 5  GA$1   $
    m = 2, n = 6, C[A] = 2, C[C] = 4, C[G] = 5.  Splitters: p0 = row 0, p1 = row 1 (the sentinel rows), p2 = row 2, p3 = row 4 (rows 2 + 2i).
    Pieces: p0 reads C at row 0 and lands on row 4 = p3: (p3, 1 step).  p1 reads A at row 1 and lands on row 2 = p2: (p2, 1).  p2 reads G at row 2,
    goes to row 5, no splitter, and reads the sentinel there: LF leads to sentinel row 1, so (string 1, 2 steps) and the end row of string 1 is 5.
    p3 reads A at row 4, goes to row 3 and reads the sentinel: (string 0, 2 steps), end row 3.
    Join: D(p2) = D(p3) = 2, D(p0) = 1 + D(p3) = 3, D(p1) = 1 + D(p2) = 3; both strings have D - 1 = 2 symbols.
    Keys (string, D - 1): p0 (0, 2), p1 (1, 2), p2 (1, 1), p3 (0, 1); sorted: p3, p0, p2, p1.
    Row 0 is splitter p0 at place 1, its string's first piece stands at place 0: pieces p3, p0; p3 writes A (d = 2) to 0, p0 writes C (d = 3) to 1: AC.
    Row 4 is splitter p3: piece p3 alone, the answer is A.  Rows 3 and 5 read the sentinel at once: D = 1, nothing, end rows 3 and 5."""
    fm = wm.Fm(np.array([2, 1, 3, 0, 1, 0], dtype=np.uint8))
    pc = pm.Pieces(fm, 1)
    assert pc.nsp == 4 and pc.row.tolist() == [0, 1, 2, 4]
    assert pc.nxt.tolist() == [3, 2, -1, -1] and pc.string.tolist() == [-1, -1, 1, 0] and pc.steps.tolist() == [1, 1, 2, 2]
    assert pc.D.tolist() == [3, 3, 2, 2] and pc.s.tolist() == [0, 1, 1, 0] and pc.end_row.tolist() == [3, 5]
    assert pc.sorted.tolist() == [3, 0, 2, 1] and pc.pos.tolist() == [1, 3, 2, 0]
    end, seqs, st = pc.retrieve([0, 1, 4, 3, 5, 2, 6, -1])
    assert end.tolist() == [3, 5, 3, 3, 5, 5, -1, -1]
    assert [wm.LETTERS[s].tobytes() for s in seqs] == [b"AC", b"GA", b"A", b"", b"", b"G", b"", b""]
    # 6 steps for the pieces, 1 each for rows 3 and 5 down to the sentinel, and D steps per row to write: 3 + 3 + 2 + 1 + 1 + 2
    assert st == {"n_pieces": 4, "max_piece_steps": 2, "n_symbols": 6, "n_rows": 8, "n_steps": 6 + 2 + 12}
    assert pm.get_text(pc, [0, 1]) == wm.get_text(fm, [0, 1]) == b">0 3\nAC\n>1 5\nGA\n"


# ---- the CLI before any device work ----

def _cli(args):
    return subprocess.run([CLI, "get"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_cli_all_takes_no_row_and_the_usage_line_stays():
    idx = os.path.join(GOLDEN, "k4_readme.fmd")
    for args in ([idx, "0", "--all"], ["--all", idx, "0"], ["--all", "--pieces", idx, "3", "4"]):
        r = _cli(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1, args
    for args in (["--all"], ["--pieces"], ["--pieces", idx], ["--all", "-1"]):
        r = _cli(args)
        assert r.returncode == 0 and r.stdout == b"Usage: ropebwt3-amd get <idx.fmr> <int> [...]\n", args
