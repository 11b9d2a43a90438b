"""BRE on the host (no GPU): the Python model against the files the unmodified reference wrote (tests/golden/*.bre,
BRE_MANIFEST.json, made by tools/make_golden_bre.py), and the host library's reader, run decoder and packer -- through the CLI's
`recode`, which uses nothing else -- against the model, with every refusal of the reader."""
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build, gpu
from tests import bre_model, util

CLI = _build.BIN_CLI
MAN = json.load(open(os.path.join(util.GOLDEN, "BRE_MANIFEST.json")))
PLAIN = sorted(f[:-7] for f in os.listdir(util.GOLDEN) if f.endswith(".bwt.gz"))
FIXTURES = sorted(f[:-4] for f in os.listdir(util.GOLDEN) if f.endswith(".bre"))


def plain_bwt(name):
    s = gzip.open(os.path.join(util.GOLDEN, name + ".bwt.gz")).read().strip()
    return np.frombuffer(s.translate(bytes.maketrans(b"$ACGTN", bytes(range(6)))), dtype=np.uint8)


def recode(args, data, tmp_path, ok=True):
    src = tmp_path / "in.bre"
    src.write_bytes(data)
    r = subprocess.run([CLI, "recode"] + args + [str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert (r.returncode == 0) == ok, r.stderr.decode()[-400:]
    return r


def test_fixture_list():
    assert len(PLAIN) >= 8 and set(FIXTURES) == {"k4_readme", "k2_fwd", "edge_chars", "edge_dups", "longruns", "copies3000"}


@pytest.mark.parametrize("name", PLAIN)
def test_model_writes_the_reference_file(name):
    data = bre_model.encode(bre_model.runs_of(plain_bwt(name)), 2)
    ent = MAN["from_fmd"][name]
    assert len(data) == ent["bytes"] and hashlib.md5(data).hexdigest() == ent["md5"]
    assert len(data) == 24 + 3 * ent["n_rec"] + 3 + 24
    if name in FIXTURES:
        assert data == open(os.path.join(util.GOLDEN, name + ".bre"), "rb").read()


@pytest.mark.parametrize("name", FIXTURES)
def test_model_reads_the_reference_file(name):
    data = open(os.path.join(util.GOLDEN, name + ".bre"), "rb").read()
    bpr, runs, counted, ftr = bre_model.decode(data)
    ent = MAN["from_fmd"][name]
    assert bpr == 2 and counted == ftr == (ent["n_rec"], ent["n_sym"], ent["n_run"])
    if name in PLAIN:
        assert runs == bre_model.runs_of(plain_bwt(name))
    assert bre_model.encode(runs, 2) == data
    assert gpu.read_bre(os.path.join(util.GOLDEN, name + ".bre")) == (2, data[24:24 + 3 * ftr[0]], ftr)


def test_longruns_splits_its_runs():
    _, runs, counted, _ = bre_model.decode(open(os.path.join(util.GOLDEN, "longruns.bre"), "rb").read())
    assert counted == (54, 2014018, 24) and max(l for _, l in runs) > 3 * 65535


@pytest.mark.parametrize("bpr", [1, 2, 4])
@pytest.mark.parametrize("name", FIXTURES + ["genomes12"])
def test_host_reader_decoder_and_packer(name, bpr, tmp_path):
    """the host reader + run decoder read the model's file (joined or not, with auxiliary bytes), the host packer writes it"""
    if name in PLAIN:
        runs = bre_model.runs_of(plain_bwt(name))
    else:
        runs = bre_model.decode(open(os.path.join(util.GOLDEN, name + ".bre"), "rb").read())[1]
    want = bre_model.encode(runs, bpr)
    plain = bytes(b"$ACGTN"[c] for c in bre_model.plain_of(runs)) + b"\n" if sum(l for _, l in runs) < 1 << 20 else None
    for data in (want, bre_model.encode(runs, bpr, joined=False), bre_model.encode(runs, bpr, aux=b"\0any\0aux")):
        assert recode(["-e", "--bre-run-bytes", str(bpr)], data, tmp_path).stdout == want
        if plain is not None:
            assert recode([], data, tmp_path).stdout == plain
    # through the other codecs and back
    fmd = recode(["-d"], want, tmp_path).stdout
    if os.path.exists(os.path.join(util.GOLDEN, name + ".fmd")):
        assert fmd == open(os.path.join(util.GOLDEN, name + ".fmd"), "rb").read()
    assert recode(["-e", "--bre-run-bytes", str(bpr)], fmd, tmp_path).stdout == want


def test_host_reader_takes_eight_length_bytes(tmp_path):
    runs = bre_model.runs_of(plain_bwt("k4_readme"))
    assert recode(["-e"], bre_model.encode(runs, 8), tmp_path).stdout == bre_model.encode(runs, 2)
    assert recode(["-e", "--bre-run-bytes", "8"], bre_model.encode(runs, 3), tmp_path).stdout == bre_model.encode(runs, 8)


def broken_files():
    """name -> a BRE file the reader must refuse (from the model's k4_readme at two length bytes)"""
    good = bre_model.encode(bre_model.runs_of(plain_bwt("k4_readme")), 2)
    n_rec = (len(good) - 24 - 3 - 24) // 3
    le = lambda x: x.to_bytes(8, "little")
    out = {
        "cut file": good[:-30],
        "no footer": good[:-27],
        "short footer": good[:-1],
        "wrong n_rec": good[:-24] + le(n_rec + 1) + good[-16:],
        "wrong n_sym": good[:-16] + le(65) + good[-8:],
        "wrong n_run": good[:-8] + le(n_rec - 1),
        "zero-length record": good[:24 + 3 * 5] + b"\x02\0\0" + good[24 + 3 * 5:-24] + le(n_rec + 1) + good[-16:],
        "asize 16": good[:8] + le(16) + good[16:],
        "b_per_sym 2": good[:4] + b"\x02" + good[5:],
        "b_per_run 0": good[:5] + b"\x00" + good[6:],
        "b_per_run 9": good[:5] + b"\x09" + good[6:],
        "symbol 6": good[:24 + 3 * 7] + b"\x06" + good[24 + 3 * 7 + 1:],
        "wrong magic": b"BRE\x02" + good[4:],
        "no records": good[:24] + bytes(3) + le(0) * 3,
        "header only": good[:20],
    }
    return out


BROKEN = broken_files()


@pytest.mark.parametrize("what", sorted(BROKEN))
def test_reader_refusals(what, tmp_path):
    r = recode(["-d"], BROKEN[what], tmp_path, ok=False)
    assert r.returncode == 1 and r.stdout == b"" and len(r.stderr.decode().strip().splitlines()) == 1
    if what not in ("wrong n_sym", "wrong n_run", "wrong magic"):   # (those two counts take the decoder; the reader alone is the Python mirror's)
        with pytest.raises(ValueError):
            gpu.read_bre(str(tmp_path / "in.bre"))


def test_write_bre_mirror(tmp_path):
    data = open(os.path.join(util.GOLDEN, "longruns.bre"), "rb").read()
    bpr, rec, counts = gpu.read_bre(os.path.join(util.GOLDEN, "longruns.bre"))
    gpu.write_bre(str(tmp_path / "x.bre"), rec, bpr, counts)
    assert (tmp_path / "x.bre").read_bytes() == data
