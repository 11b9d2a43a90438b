"""hapdiv without a GPU: what tests/golden/HAPDIV_MANIFEST.json must hold; the Python model of the dynamic program (tests/sw_model.py)
against the reference's committed output, window by window; the model's table through a growth; the merging of windows into lines."""
import json
import os

import numpy as np
import pytest

from ropebwt3_amd import _build
from ropebwt3_amd.gpu import hapdiv_lines
from tests import kount_model as km
from tests import mem_model as mm
from tests import sw_model as sw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "HAPDIV_MANIFEST.json")))
STDOUT = json.load(open(os.path.join(GOLDEN, "HAPDIV_STDOUT.json")))
SYMMETRIC = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
             "edge_dups.fmd", "longruns.fmd", "copies3000.fmd"]
OPT_OF = {"-N": "n_best", "-m": "min_sc", "-A": "match", "-B": "mis", "-O": "gap_open", "-E": "gap_ext", "-y": "e2e_drop"}


def test_manifest_is_complete():
    for key, e in MANIFEST.items():
        assert key == " ".join(e["opts"] + e["files"]) and len(e["md5"]) == 32 and e["lines"] >= 0
        for f in e["files"]:
            assert os.path.exists(os.path.join(GOLDEN, f)), f
        assert ("model" in e) == (key in STDOUT)
    for idx in SYMMETRIC:
        for q in ("mem_mutated.fa.gz", "mem_iupac.fa", "reads_fq.fa.gz", "-L edge_chars.txt"):
            for o in ("", "-a31 -w7", "-a51 -w10 -N5", "-a31 -w1 -N3", "-N1"):
                qo, qf = (q.split() if " " in q else ("", q))
                key = " ".join(x for x in (o, qo, idx, qf) if x)
                assert key in MANIFEST and MANIFEST[key]["matrix"], key
    g = "genomes12.fmd mem_mutated.fa.gz"
    for o in ("-N200", "-a1 -w1", "-m1 -a20", "-y2", "-y0", "-A2 -B4 -O4 -E1", "-a5000", "-K1k"):
        assert MANIFEST[o + " " + g]["lines"] > 0, o
    assert MANIFEST["-K1k " + g]["md5"] == MANIFEST[g]["md5"]                      # a batch holds whole queries
    assert MANIFEST[g]["lines"] == 788 and MANIFEST["-a51 -w10 -N5 " + g]["lines"] == 3121
    assert MANIFEST["-a31 -w7 reads_fq.fmd reads_fq.fa.gz"]["lines"] == 18577
    assert MANIFEST["-e -k5 -b -u -j30 -l40 --seq " + g]["md5"] == MANIFEST[g]["md5"]   # accepted, and they change nothing
    assert sum(1 for e in MANIFEST.values() if len(e["files"]) > 2) >= 3
    refused = [e for e in MANIFEST.values() if "refused" in e]
    assert len(refused) == 3 and all(e["lines"] == 0 and e["refused"] == "ERROR: BWT doesn't contain both strands" for e in refused)
    model = [e for e in MANIFEST.values() if e.get("model")]
    assert any("-N1" in e["opts"] for e in model) and any("-N3" in e["opts"] or "-N5" in e["opts"] for e in model)
    assert any("mem_iupac.fa" in e["files"] for e in model) and any("-O4" in e["opts"] for e in model)


def _model_args(e):
    k, w, o = 101, 50, {}
    for x in e["opts"]:
        if x.startswith("-a"):
            k = int(x[2:])
        elif x.startswith("-w"):
            w = int(x[2:])
        elif x[:2] in OPT_OF:
            o[OPT_OF[x[:2]]] = int(x[2:])
    return k, w, o


_INDEXES = {}


def _index(name):
    if name not in _INDEXES:
        _INDEXES[name] = sw.BwtIndex(km.golden_plain(GOLDEN, name, _build.BIN_CLI))
    return _INDEXES[name]


@pytest.mark.parametrize("key", sorted(STDOUT))
def test_model_reproduces_reference(key):
    """every window of the committed cases: the model's nine numbers, merged into lines, are the reference's bytes -- and unmerged, every
    window agrees with the line that covers it"""
    e = MANIFEST[key]
    k, w, o = _model_args(e)
    qs = mm.read_queries(os.path.join(GOLDEN, e["files"][1]), "-L" in e["opts"])
    wins = sw.hapdiv(_index(e["files"][0]), [mm.nt6(s) for _, s in qs], k, w, o)
    want = STDOUT[key].encode()
    assert sw.merge_lines(wins, k, [n for n, _ in qs]) == want
    lines = [l.split(b"\t") for l in want.splitlines()]
    names = [(n.encode() if n is not None else b"seq%d" % (i + 1)) for i, (n, _) in enumerate(qs)]
    for q, off, nine in wins:
        cover = [l for l in lines if l[0] == names[q] and int(l[1]) <= off and off + k <= int(l[2]) and (off - int(l[1])) % w == 0]
        assert len(cover) == 1 and tuple(int(x) for x in cover[0][3:]) == tuple(nine), (q, off)


def test_table_growth_keeps_the_reference_slots():
    """a table made for n_best 2 has 8 slots and doubles when a put finds 6 entries: the slots before and after, worked out by hand from
    the hash -- every key's home slot, linear probing, and at the growth the old entries re-placed in slot order, each into the first
    free slot from its new home"""
    t = sw.SlotTable(2 * 4)
    assert t.bits == 3 and len(t.slots) == 8
    keys = [(10 * i + 3, 10 * i + 8) for i in range(9)]
    want = {}
    for lo, hi in keys[:6]:
        s = sw.home_slot(sw.key_hash(lo, hi), 3)
        while s in want.values():
            s = (s + 1) & 7
        want[(lo, hi)] = s
        slot, absent = t.put(sw.Cell(lo, hi, 0, H=lo))
        assert absent and slot == s
    assert t.count == 6 and t.grown == 0 and sorted(t.occupied()) == sorted(want.values())
    slot, absent = t.put(sw.Cell(keys[2][0], keys[2][1], 0, H=99))
    assert not absent and slot == t.find(*keys[2])
    assert t.grown == 1 and t.bits == 4 and t.count == 6                     # the growth comes before the probe, even for a key that is there
    # the re-placement, replayed on plain lists: old entries in slot order; one whose new slot holds an old entry displaces it
    old = {s: key for key, s in want.items()}
    new, pending = {}, dict(old)
    for j in range(8):
        if j not in pending:
            continue
        cur = pending.pop(j)
        while True:
            i = sw.home_slot(sw.key_hash(*cur), 4)
            while i in new:
                i = (i + 1) & 15
            new[i] = cur
            if i in pending:
                cur = pending.pop(i)
            else:
                break
    assert {i: (t.slots[i].lo, t.slots[i].hi) for i in t.occupied()} == new
    assert t.slots[t.find(*keys[2])].H == keys[2][0]                         # a put of a key that is there stores nothing
    for lo, hi in keys[6:]:
        assert t.put(sw.Cell(lo, hi, 0))[1]
    assert t.count == 9 and t.grown == 1
    t.clear()
    assert t.bits == 4 and t.count == 0 and t.occupied() == []               # the capacity stays for the next row
    # ties in H: the higher slot comes first
    a, b = sw.Cell(1, 2, 0, H=5), sw.Cell(3, 4, 0, H=5)
    sa, sb = t.put(a)[0], t.put(b)[0]
    top = sw.top_cells(t, 1)
    assert (top[0].lo, top[0].hi) == ((1, 2) if sa > sb else (3, 4))


def test_merge_is_strict():
    t = sw.SlotTable(8)
    first = sw.Cell(1, 9, 0, H=7, H_pos=11)
    assert sw.merge(t, first)[1] == 7
    q, ch = sw.merge(t, sw.Cell(1, 9, 5, H=7, H_pos=22))
    assert ch == 0 and q.H_pos == 11 and q.lo_rc == 0                        # the first arrival keeps a tie
    q, ch = sw.merge(t, sw.Cell(1, 9, 5, H=8, E=8, H_from=sw.FROM_E, E_from=sw.EXT, E_pos=33))
    assert ch == 3 and q.H == 8 and q.H_from == sw.FROM_E and q.H_pos == 11 and q.E_pos == 33   # H_pos follows a winner from H only


def test_line_merger():
    z, a, b = (0,) * 9, (1, 0, 3, 0, 0, 0, 0, 0, 0), (2, 1, 3, 4, 0, 0, 0, 0, 0)
    wins = [(0, 0, a), (0, 5, a), (0, 10, b), (0, 15, a), (1, 0, a), (1, 5, z), (1, 10, z), (3, 0, z)]
    want = (b"q0\t0\t15\t1\t0\t3\t0\t0\t0\t0\t0\t0\n" b"q0\t10\t20\t2\t1\t3\t4\t0\t0\t0\t0\t0\n" b"q0\t15\t25\t1\t0\t3\t0\t0\t0\t0\t0\t0\n"
            b"seq9\t0\t10\t1\t0\t3\t0\t0\t0\t0\t0\t0\n" b"seq9\t5\t20\t0\t0\t0\t0\t0\t0\t0\t0\t0\n" b"seq11\t0\t10\t0\t0\t0\t0\t0\t0\t0\t0\t0\n")
    names = ["q0", None, "unused", None]
    assert sw.merge_lines(wins, 10, names, first_id=7) == want
    recs = np.array([x[2] for x in wins], dtype=np.int32)
    where = np.array([x[:2] for x in wins], dtype=np.int64)
    assert hapdiv_lines(recs, where, 10, names, first_id=7) == want
    assert hapdiv_lines(recs[:0], where[:0], 10) == b"" and sw.merge_lines([], 10) == b""
