"""kount without a device: the Python model (tests/kount_model.py) against the reference binary and the recorded goldens, the
order rule on the README example, and the CLI's refusals that come before any device work."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import util
from tests import kount_model as km

CLI = _build.BIN_CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "KOUNT_MANIFEST.json")))


def _ref_kount(args):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    r = subprocess.run([util.REF_BIN, "kount"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


def _model(names, k, m):
    return km.lines(*km.kount([km.golden_plain(GOLDEN, f, CLI) for f in names], k, m))


@pytest.mark.parametrize("names", [["k4_readme.fmd"], ["edge_chars.fmd"], ["edge_dups.fmd"], ["reads_fwd.fmd"], ["k3_both.fmd", "k2_fwd.fmd"],
                                   ["reads_fwd.fmd", "edge_chars.fmd"]])
@pytest.mark.parametrize("k,m", [(1, 1), (3, 1), (5, 2), (12, 2), (31, 1), (31, 3), (2, 0), (4, -1)])
def test_model_matches_reference(names, k, m):
    got = _model(names, k, m)
    assert got == _ref_kount(["-k%d" % k, "-m%d" % m] + [os.path.join(GOLDEN, f) for f in names])


@pytest.mark.parametrize("key", ["-k31 -m2 genomes12.fmd", "-k80 -m3 genomes12.fmd", "-k51 -m2 reads_fq.fmd", "-k6 -m0 k2_fwd.fmd",
                                 "-k25 -m2 genomes12_first6.fmr reads_fq.fmd edge_chars.fmd", "-k17 -m3 reads_fwd.fmd reads_rev.fmd",
                                 "-k4 -m1 k4_readme.fmd k3_both.fmd k2_fwd.fmd", "-k12 -m1000000000 genomes12.fmd", "-k1 -m100 reads_rev.fmd",
                                 "-k3 -m2 longruns.fmd", "-k80 -m1 edge_dups.fmd", "-k31 -m2 copies3000.fmd"])
def test_model_matches_recorded(key):
    e = MANIFEST[key]
    args = e["args"]
    got = _model(args[2:], int(args[0][2:]), int(args[1][2:]))
    assert got.count(b"\n") == e["lines"]
    assert hashlib.md5(got).hexdigest() == e["md5"]


def test_issue_table_recorded():
    """the known answers of the unmodified reference are what the manifest holds"""
    want = {"-k31 -m2 genomes12.fmd": (40432, "bb73b1be70a02f0c4389e12ead1682ea"),
            "-k80 -m3 genomes12.fmd": (39842, "be5313c9d326c6616a64b2cc7dd66ce8"),
            "-k51 -m2 reads_fq.fmd": (53922, "e63531a173c48841439657386d44b2fb"),
            "-k25 -m2 genomes12_first6.fmr reads_fq.fmd edge_chars.fmd": (101498, "100f5c7cea0cfda2f5563aba711dc0a8"),
            "-k6 -m0 k2_fwd.fmd": (4096, "cc5d0a53b48333b78b329a13b1acd1f9")}
    for key, (n, md5) in want.items():
        assert (MANIFEST[key]["lines"], MANIFEST[key]["md5"]) == (n, md5), key


def test_order_rule_readme_example():
    kmers, counts = km.kount([km.golden_plain(GOLDEN, "k4_readme.fmd", CLI)], 3, 1)
    first = [bytes(b"$ACGTN"[c] for c in s).decode() for s in kmers[:12]]
    assert first == "ATT CTT GTT TTT AGT GGT TGT ACT TCT AAT CAT TAT".split()


def test_order_rule_is_the_trie_walk():
    """the sort rule equals a depth-first walk that pushes children A..T (so visits T..A) and prints the last level A..T"""
    k = 4
    alls = np.array(np.meshgrid(*[np.arange(1, 5)] * k, indexing="ij")).reshape(k, -1).T.astype(np.uint8)
    got = [tuple(x) for x in alls[km.order(alls)]]
    want = []

    def walk(suffix):  # the symbols chosen at depth 1, 2, ...: the last character first
        if len(suffix) == k - 1:
            want.extend((a,) + tuple(reversed(suffix)) for a in range(1, 5))
            return
        for a in range(4, 0, -1):
            walk(suffix + [a])
    walk([])
    assert got == want


def test_cli_refusals_without_device():
    r = subprocess.run([CLI, "kount"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr
    r = subprocess.run([CLI, "kount", "-k0", os.path.join(GOLDEN, "k4_readme.fmd")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b""
    r = subprocess.run([CLI, "kount", "-k", "-3", os.path.join(GOLDEN, "k4_readme.fmd")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b""
