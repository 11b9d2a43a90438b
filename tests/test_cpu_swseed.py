"""sw --prefilter without a GPU: the model of the reference's MEM pre-filter (tests/seed_model.py) against the reference's committed output
-- a filtered answer is its unfiltered twin with the lines of the queries without a seed taken out (with -u: turned into unmapped lines)
--, against brute force on small random indexes, and on a hand-worked example whose steps are counted; what
tests/golden/SWSEED_MANIFEST.json must hold; the refusals that need no device."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, host
from tests import kount_model as km
from tests import mem_model as mm
from tests import seed_model as sm
from tests import sw_model as sw
from tests import swaln_model as sa
from tests import util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "SWSEED_MANIFEST.json")))
STDOUT = json.load(open(os.path.join(GOLDEN, "SWSEED_STDOUT.json")))
G8 = "-s8 %s genomes12.fmd sw_reads.fa"
BITES = {"-e -j20": (911, 919), "-e -j30": (834, 919), "-e -j60": (381, 919), "-e -j100": (102, 919), "-e -u -j30": (889, None), "-e -k5 -j25": (888, None),
         "-j20": (214, 216), "-j40": (147, 216), "-u -j40": (241, None), "-k5 -j30": (188, None), "-g2 -b -j30": (1476, 1546)}


def _key(e):
    return ("" if e["S"] is None else "-s%d " % e["S"]) + " ".join(e["opts"] + e["files"])


def _min_len(e):
    return int([o for o in e["opts"] if o.startswith("-j")][0][2:])


def test_manifest_is_complete():
    for key, e in MANIFEST.items():
        assert key == _key(e) and len(e["md5"]) == 32 and len(e["twin_md5"]) == 32
        for f in e["files"]:
            assert os.path.exists(os.path.join(GOLDEN, f)), f
        assert "--prefilter" not in e["opts"] and "--local" not in e["opts"]           # the reference's own options
        assert sum(1 for o in e["opts"] if o.startswith("-j")) == 1
        assert e["twin"] == _key(dict(e, opts=[o for o in e["opts"] if not o.startswith("-j")]))
        assert e.get("model", False) == (key in STDOUT) and (not e.get("model") or e["twin"] in STDOUT)
        if e["bites"]:
            assert e["lines"] > 0 and e["md5"] != e["twin_md5"], key
    for o, (lines, twin) in BITES.items():                                             # the biting cases on the read fixture
        e = MANIFEST[G8 % o]
        assert e["bites"] and e["lines"] == lines and (twin is None or e["twin_lines"] == twin), o
    sw_man = json.load(open(os.path.join(GOLDEN, "SW_MANIFEST.json")))
    swl_man = json.load(open(os.path.join(GOLDEN, "SWLOCAL_MANIFEST.json")))
    assert MANIFEST[G8 % "-e -j20"]["twin_md5"] == sw_man[G8 % "-e"]["md5"] and MANIFEST[G8 % "-j20"]["twin_md5"] == swl_man["-s8 genomes12.fmd sw_reads.fa"]["md5"]
    for o in ("-e -p3 -j30", "-p3 -j40", "-e -K1k -j30", "-K1k -j40"):
        assert MANIFEST[G8 % o]["bites"], o
    assert MANIFEST[G8 % "-e -K1k -j30"]["md5"] == MANIFEST[G8 % "-e -j30"]["md5"] and MANIFEST[G8 % "-K1k -j40"]["md5"] == MANIFEST[G8 % "-j40"]["md5"]
    assert sum(1 for e in MANIFEST.values() if len(e["files"]) > 2) >= 2
    for j in (20, 30):
        for o in ("-L -e -j%d", "-L -e -u -j%d", "-L -j%d", "-L -u -j%d"):
            e = MANIFEST["-s8 " + o % j + " genomes12.fmd seed_lines.txt"]
            assert e["bites"] and e.get("model"), (o, j)
    for o in ("-e -j30", "-j30"):
        e = MANIFEST["-s8 %s genomes12.fmd mem_mutated.fa.gz" % o]
        assert e["lines"] > 0 and e["md5"] == e["twin_md5"]                            # queries of kilobases: all pass
    for at, above in (("-e -k5 -j5", "-e -k5 -j6"), ("-k11 -j11", "-k11 -j12")):
        assert MANIFEST[G8 % at]["md5"] == MANIFEST[G8 % at]["twin_md5"] and MANIFEST[G8 % above]["lines"] > 0
    others = [e for e in MANIFEST.values() if e["files"][0] != "genomes12.fmd" and e["opts"] == ["-e", "-j30"] and e["files"][1:] == ["sw_reads.fa"]]
    assert len(others) >= 3 and any(0 < e["lines"] < e["twin_lines"] for e in others)


def test_seed_lines_fixture():
    ls = [s for _, s in mm.read_queries(os.path.join(GOLDEN, "seed_lines.txt"), True)]
    assert 24 <= len(ls) <= 60 and max(len(l) for l in ls) <= 300
    at = ls.index(b"")
    assert 0 < at < len(ls) - 1 and ls[at - 1] and ls[at + 1]                        # an empty line between two others
    assert any(l and set(l) == {ord("N")} for l in ls) and sum(1 for l in ls if 0 < len(l) < 20) >= 2


_INDEXES = {}


def _index(name):
    if name not in _INDEXES:
        _INDEXES[name] = sw.BwtIndex(km.golden_plain(GOLDEN, name, _build.BIN_CLI))
    return _INDEXES[name]


@pytest.mark.parametrize("key", sorted(k for k, e in MANIFEST.items() if e.get("model")))
def test_model_selects_the_lines_of_the_reference(key):
    """the recorded answer with -j is the recorded answer without it, keeping the lines of the queries for which the model finds a seed; with -u
    the others get the unmapped line.  This pins the model to the reference"""
    e = MANIFEST[key]
    ix = _index(e["files"][0])
    unmapped, min_len = "-u" in e["opts"], _min_len(e)
    per = {}
    for line in STDOUT[e["twin"]].splitlines(True):
        per.setdefault(line.split("\t")[0], []).append(line)
    want, qid, n_out, kinds = [], 0, 0, set()
    for fn in e["files"][1:]:
        for name, s in mm.read_queries(os.path.join(GOLDEN, fn), "-L" in e["opts"]):
            q = mm.nt6(s)
            p, _ = sm.present(ix, q, min_len)
            assert p == sm.present_chunked(ix, q, min_len, 7)
            mine = per.get(sa._name(name, qid), [])
            mapped = [l for l in mine if l.split("\t")[2] != "*"]
            if p:
                want += mine
            elif unmapped:
                want.append(sa.unmapped_line(name, qid, q).decode())
            n_out += (not p) and bool(mapped)
            kinds.add((p, bool(mapped)))
            qid += 1
    assert "".join(want) == STDOUT[key]
    assert n_out > 0                                     # the filter took out a query that has a hit without it
    if "seed_lines.txt" in e["files"]:
        assert kinds >= {(1, True), (0, True), (0, False)}


def _brute_index(rng, n_str, length, with_n):
    recs = []
    for _ in range(n_str):
        s = rng.integers(1, 5, size=int(rng.integers(1, length + 1))).astype(np.uint8)
        if with_n and s.size > 4:
            at = int(rng.integers(0, s.size - 2))
            s[at:at + int(rng.integers(1, 4))] = 5
        recs.append(s)
    return recs


def test_model_matches_brute_force():
    rng = np.random.default_rng(11)
    seen = set()
    for trial in range(40):
        recs = _brute_index(rng, int(rng.integers(1, 5)), 40, trial % 2 == 1)
        both = trial % 4 != 3                            # a forward-only index serves as well
        ix = sw.BwtIndex(host.build_bwt(util.make_text(recs, rev=both)))
        strings = [r.tolist() for r in recs] + ([util.revcomp(r).tolist() for r in recs] if both else [])
        for _ in range(40):
            kind = int(rng.integers(0, 4))
            if kind == 0:                                # random: mostly absent
                q = rng.integers(1, 6, size=int(rng.integers(0, 30))).astype(np.uint8)
            else:                                        # a piece of a record between random flanks, some symbols turned into N
                r = recs[int(rng.integers(0, len(recs)))]
                a = int(rng.integers(0, r.size))
                q = np.concatenate([rng.integers(1, 5, size=int(rng.integers(0, 6))).astype(np.uint8), r[a:a + int(rng.integers(1, 12))],
                                    rng.integers(1, 5, size=int(rng.integers(0, 6))).astype(np.uint8)])
                if kind == 3 and q.size:
                    q[int(rng.integers(0, q.size))] = 5
            for min_len in (2, 3, 5, 9):
                p, steps = sm.present(ix, q, min_len)
                assert p == sm.brute(strings, q, min_len), (trial, q.tolist(), min_len)
                assert p == sm.present_chunked(ix, q, min_len, 1) == sm.present_chunked(ix, q, min_len, 3)
                assert (steps == 0) == (len(q) < min_len)
                seen.add((p, 5 in q.tolist(), len(q) < min_len))
    assert {(1, True, False), (0, True, False), (1, False, False), (0, False, False), (0, False, True)} <= seen


def test_hand_worked_steps():
    """GATTACA and its reverse complement TGTAATC, windows of 4 symbols.
    CACGGATTAC: window 0 = CACG starts from G; C: CG does not occur (step 1), so windows 1 and 2, which hold CG, are skipped and window 3 = GGAT
    starts from T; A: AT occurs (2); G: GAT occurs (3); G: GGAT does not (4), next window 4 = GATT from T; T: TT (5); A: ATT (6); G: GATT (7): a seed
    after 7 steps, where a scan of the windows 0..4 one by one takes 1 + 1 + 2 + 3 + 3 = 10.
    CACGGATCAC: the same four steps, then window 4 = GATC from C; T: TC occurs (5); A: ATC occurs (6); G: GATC does not (7), window 5 = ATCA from A;
    C: CA occurs (8); T: TCA does not (9), window 7 has three symbols: no seed after 9 steps."""
    s = mm.nt6(b"GATTACA")
    ix = sw.BwtIndex(host.build_bwt(util.make_text([s])))
    assert sm.present(ix, mm.nt6(b"CACGGATTAC"), 4) == (1, 7)
    assert sm.present(ix, mm.nt6(b"CACGGATCAC"), 4) == (0, 9)
    assert sm.present(ix, mm.nt6(b"GAT"), 4) == (0, 0) and sm.present(ix, mm.nt6(b""), 4) == (0, 0)
    assert sm.present(ix, mm.nt6(b"CACGGATTAC"), 4, 0, 3) == (0, 1) and sm.present(ix, mm.nt6(b"CACGGATTAC"), 4, 3, 7) == (1, 6)   # two walkers


def test_cli_still_refuses_without_prefilter():
    """-j above the end length without --prefilter: one line on stderr, nothing on stdout, exit 1, before any device is opened"""
    cli = _build.BIN_CLI
    idx, q = os.path.join(GOLDEN, "genomes12.fmd"), os.path.join(GOLDEN, "mem_iupac.fa")
    for bad in (["-e", "-j2"], ["--local", "-j12"], ["--local", "-k5", "-j6"], ["-g2", "-j30"]):
        r = subprocess.run([cli, "sw"] + bad + [idx, q], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"\n") == 1 and b"--prefilter" in r.stderr, bad
    u = subprocess.run([cli, "sw"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert u.returncode == 0 and b"--prefilter" in u.stderr and b"-j INT" in u.stderr


def test_abi_symbol():
    lib = ctypes.CDLL(_build.LIB_GPU)
    assert hasattr(lib, "rb3gpu_seed_present")
