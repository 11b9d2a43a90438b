"""`remove` without a GPU: walk, mark and compact restated in numpy (tests/remove_model.py) over the committed plain BWTs against the committed
indexes, the oracle's BWT of the strings that stay and the reference's recorded answers (tests/golden/REMOVE_MANIFEST.json); the parser of the
command's arguments in C and in the model; what the library and the command line must offer."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, host
from ropebwt3_amd.gpu import nt6_of
from tests import kount_model as km
from tests import remove_model as rm
from tests import util

CLI = _build.BIN_CLI
GOLDEN = util.GOLDEN
MANIFEST = json.load(open(os.path.join(GOLDEN, "REMOVE_MANIFEST.json")))
INDEXES = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
WITH_PLAIN = sorted(k for k, e in MANIFEST.items() if os.path.exists(os.path.join(GOLDEN, os.path.splitext(e["index"])[0] + ".bwt.gz")))

_PLAIN = {}


def _plain(idx):
    if idx not in _PLAIN:
        _PLAIN[idx] = km.read_plain(os.path.join(GOLDEN, os.path.splitext(idx)[0] + ".bwt.gz"))
    return _PLAIN[idx]


def _rows(e):
    return [r for a, b in e["rows"] for r in range(a, b + 1)]


def _strands(name):
    """the strings of a committed index of lines, in the order of its rows"""
    e = INDEXES[name]
    fwd, rev = "-F" not in e["flags"], "-R" not in e["flags"]
    out = []
    for line in open(os.path.join(GOLDEN, e["inputs"][0])).read().split("\n"):
        if line.strip():
            s = nt6_of(line.strip())
            out += ([s] if fwd else []) + ([util.revcomp(s)] if rev else [])
    return out


def test_manifest_holds_data_only():
    assert len(MANIFEST) >= 40
    for k, e in MANIFEST.items():
        assert sorted(e) == ["bytes", "case", "index", "md5", "rows"] and k.endswith("/" + e["case"])
        assert os.path.exists(os.path.join(GOLDEN, e["index"])) and len(e["md5"]) == 32 and e["bytes"] > 0
        assert all(len(r) == 2 and 0 <= r[0] <= r[1] for r in e["rows"])
    covered = {e["index"] for e in MANIFEST.values()}
    assert {x + ".fmd" for x in ("edge_chars", "edge_dups", "k2_fwd", "k3_both", "k4_readme", "copies3000", "longruns", "reads_fwd", "reads_rev", "reads_fq")} <= covered


def test_genomes12_without_its_last_six_is_the_committed_index():
    r = subprocess.run([CLI, "recode", os.path.join(GOLDEN, "genomes12_first6.fmd")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, check=True)
    want = np.frombuffer(r.stdout.rstrip(b"\n"), dtype=np.uint8)
    got, gone = rm.remove(_plain("genomes12.fmd"), range(12, 24))
    assert bytes(b"$ACGTN"[x] for x in got[:64]) == want[:64].tobytes()
    assert np.array_equal(np.frombuffer(b"$ACGTN", dtype=np.uint8)[got], want)
    assert gone[0] == 12 and gone.sum() == 480024 - want.size
    assert hashlib.md5(open(os.path.join(GOLDEN, "genomes12_first6.fmd"), "rb").read()).hexdigest() == MANIFEST["genomes12/rest6"]["md5"]


@pytest.mark.parametrize("name", ["edge_dups", "k3_both", "k2_fwd"])
def test_small_indexes_against_the_oracle(name):
    """every single string taken out, and all but one: duplicates (edge_dups), ties between the sentinels, one strand of a pair"""
    orc = util.Oracle()
    b = _plain(name + ".fmd")
    strs = _strands(name)
    m = len(strs)
    assert m == int((b == 0).sum()) and np.array_equal(orc.bwt(util.make_text(strs, rev=False)), b)
    for gone in [[r] for r in range(m)] + [[r for r in range(m) if r != keep] for keep in range(m)]:
        if len(gone) == m:
            continue
        got, cnt = rm.remove(b, gone + gone[:1])       # (a duplicate collapses)
        want = orc.bwt(util.make_text([s for r, s in enumerate(strs) if r not in gone], rev=False))
        assert np.array_equal(got, want), (name, gone)
        assert cnt.tolist() == (np.bincount(b, minlength=6) - np.bincount(want, minlength=6)).tolist()
    with pytest.raises(ValueError):
        rm.remove(b, range(m))
    with pytest.raises(ValueError):
        rm.remove(b, [m])


@pytest.mark.parametrize("key", WITH_PLAIN)
def test_model_gives_the_references_bytes(key):
    """the model's BWT, through the host's FMD writer, is the file the reference built from the sequences that stay"""
    e = MANIFEST[key]
    got, _ = rm.remove(_plain(e["index"]), _rows(e))
    fmd = host.fmd_bytes_from_plain(got.tobytes())
    assert len(fmd) == e["bytes"] and hashlib.md5(fmd).hexdigest() == e["md5"]


def test_compaction_positions_cross_groups():
    """the rank of the compaction: marked rows per group of 8192, new position = row - marked rows in front; a select at any new position finds its row"""
    rng = np.random.default_rng(3)
    marked = rng.random(3 * 8192 + 77) < 0.3
    marked[8191:8193] = True
    marked[16384] = False
    pre, rows, pos = rm.compact_positions(marked)
    assert pre.size == 5 and pre[0] == 0 and pre[-1] == marked.sum() and np.array_equal(pos, np.arange(rows.size))
    kept = np.minimum(np.arange(5) * 8192, marked.size) - pre           # rows kept in front of every group: what the range source searches
    for p in (0, 1, 8191, 8192, rows.size - 1):
        g = int(np.searchsorted(kept, p, side="right")) - 1
        assert g * 8192 <= rows[p] and kept[g] <= p
        assert rows[p] < (g + 1) * 8192 or kept[g + 1] <= p


ARGS = [("0", (0, 0)), ("17", (17, 17)), ("3-9", (3, 9)), ("5-5", (5, 5)), ("007", (7, 7)), ("12-0023", (12, 23)), ("288230376151711744", (288230376151711744, 288230376151711744)),
        ("", None), ("-", None), ("-3", None), ("3-", None), ("9-3", None), ("3-9-12", None), ("abc", None), ("3x", None), (" 3", None), ("3 ", None), ("+3", None), ("3..9", None),
        ("0x10", None), ("1e3", None), ("3--9", None), ("99999999999999999999", None), ("1-99999999999999999999", None)]


@pytest.mark.parametrize("arg,want", ARGS)
def test_argument_parser(arg, want):
    assert rm.parse_rows(arg) == want
    assert host.parse_rows(arg) == want


def test_expand_refuses_what_the_command_refuses():
    assert rm.expand(["1", "3-4"], 6) == [1, 3, 4] and rm.expand(["1", "0-0"], 6, pair=True) == [2, 3, 0, 1]
    for args, n, pair in ((["6"], 6, False), (["3"], 6, True), (["2-6"], 6, False), ([], 6, False), (["x"], 6, False)):
        with pytest.raises(ValueError):
            rm.expand(args, n, pair)


def test_library_exports_remove():
    lib = ctypes.CDLL(_build.LIB_GPU)
    assert hasattr(lib, "rb3gpu_remove")
    from ropebwt3_amd import gpu
    assert "rb3gpu_remove" in gpu.SYMBOLS and ctypes.sizeof(gpu.RemoveStats) == 3 * 8 + 11 * 8 and hasattr(gpu.Rb3Gpu, "remove")


def test_usage_lists_remove():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and any(line.split()[:1] == [b"remove"] for line in r.stdout.splitlines())
    r = subprocess.run([CLI, "remove"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and b"remove" in r.stderr and b"--pieces" in r.stderr and b"--pair" in r.stderr
