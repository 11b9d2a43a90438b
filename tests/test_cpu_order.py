"""build -s / -r (sorted string orders) without a device: the model the GPU path is built on, pinned against the
reference binary, and the CLI's refusals (they come before any device work)."""
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import util
from tests import order_model as om

CLI = _build.BIN_CLI


def _ref(args, tmp_path=None):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    r = subprocess.run([util.REF_BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


def _plain(out):
    """the reference's plain output ($ACGTN, one line) as symbols"""
    s = out.rstrip(b"\n")
    return np.frombuffer(s.translate(bytes.maketrans(b"$ACGTN", bytes(range(6)))), dtype=np.uint8)


def _write(path, strings, fasta=False):
    with open(path, "w") as f:
        if fasta:
            for i, s in enumerate(strings):
                f.write(">r%d\n%s\n" % (i, "".join("$ACGTN"[c] for c in s)))
        else:
            f.write(om.to_lines(strings))
    return str(path)


def _text(strings, flags):
    return util.make_text(strings, fwd="-F" not in flags, rev="-R" not in flags)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("opt", ["-s", "-r"])
@pytest.mark.parametrize("flags", [[], ["-R"], ["-F"]])
def test_order_model_matches_reference(tmp_path, oracle, seed, opt, flags):
    rng = np.random.default_rng(seed)
    strings = om.random_collection(rng, 300)
    fn = _write(tmp_path / "a.txt", strings)
    got = _plain(_ref(["build", opt, "-L"] + flags + [fn]))
    so = om.SO_RLO if opt == "-s" else om.SO_RCLO
    want = oracle.bwt(om.ordered_text(_text(strings, flags), so))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("opt", ["-s", "-r"])
def test_order_model_files_and_batches(tmp_path, oracle, opt):
    """several FASTA files, many batches (-m 5k): the result depends only on the multiset of strings"""
    rng = np.random.default_rng(7)
    so = om.SO_RLO if opt == "-s" else om.SO_RCLO
    g = util.random_genome(rng, 3000)
    parts = [util.reads_from(rng, g, 150, int(rng.integers(20, 120)), err=0.01) for _ in range(3)]
    parts[1] += om.random_collection(rng, 50)
    fns = [_write(tmp_path / ("f%d.fa" % i), p, fasta=True) for i, p in enumerate(parts)]
    got = _plain(_ref(["build", opt, "-m", "5k"] + fns))
    allstr = [s for p in parts for s in p]
    assert np.array_equal(got, oracle.bwt(om.ordered_text(_text(allstr, []), so)))


@pytest.mark.parametrize("opt", ["-s", "-r"])
def test_order_model_incremental(tmp_path, oracle, opt):
    """-i of an FMR made in the order: the union, in the order of the FMR's header byte (whichever of -s / -r is given)"""
    rng = np.random.default_rng(11)
    so = om.SO_RLO if opt == "-s" else om.SO_RCLO
    a, b = om.random_collection(rng, 200), om.random_collection(rng, 200)
    fa, fb = _write(tmp_path / "a.txt", a), _write(tmp_path / "b.txt", b)
    fmr = tmp_path / "a.fmr"
    fmr.write_bytes(_ref(["build", opt, "-b", "-L", fa]))
    assert fmr.read_bytes()[:4] == b"RB\2" + bytes([so])
    other = "-r" if opt == "-s" else "-s"
    for o in (opt, other):
        got = _plain(_ref(["build", o, "-L", "-i", str(fmr), fb]))
        assert np.array_equal(got, oracle.bwt(om.ordered_text(_text(a + b, []), so)))


def test_order_model_input_order_cases(tmp_path):
    """-i of an FMD, and an explicit -p N with one file and -t > N: the reference builds in input order"""
    rng = np.random.default_rng(5)
    a, b = om.random_collection(rng, 200), om.random_collection(rng, 200)
    fa, fb = _write(tmp_path / "a.txt", a), _write(tmp_path / "b.txt", b)
    fmd = tmp_path / "a.fmd"
    fmd.write_bytes(_ref(["build", "-d", "-L", fa]))
    io = _ref(["build", "-L", "-i", str(fmd), fb])
    assert _ref(["build", "-s", "-L", "-i", str(fmd), fb]) == io
    assert _ref(["build", "-r", "-L", "-p1", "-t4", fa]) == _ref(["build", "-L", fa])
    assert _ref(["build", "-r", "-L", "-p1", "-t4", fa, fb]) != _ref(["build", "-L", fa, fb])   # (two files: the order holds)


def test_p0_model():
    rng = np.random.default_rng(3)
    old, new = om.random_collection(rng, 100), om.random_collection(rng, 100)
    for so in (om.SO_RLO, om.SO_RCLO):
        new_o = om.ordered(new, so)
        p = om.p0(old, new_o, so)
        assert np.all(np.diff(p) >= 0) and p[0] >= 0 and p[-1] <= len(old)
        allk = sorted(om.key(s, so) for s in old)
        for s, v in zip(new_o, p):
            assert sum(k < om.key(s, so) for k in allk) == v


@pytest.mark.parametrize("args,what", [
    (["-s", "--gpus", "2"], b"--gpus"),
    (["-r", "--gpus", "2", "--interval"], b"--interval"),
    (["-s", "--host-sort"], b"--host-sort"),
    (["-r", "--host-sort", "-d"], b"--host-sort"),
])
def test_order_cli_refusals(args, what):
    """refused with a clear message before any device work (this machine may have none)"""
    r = subprocess.run([CLI, "build"] + args + ["-L", os.path.join(util.GOLDEN, "k2_fwd.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and what in r.stderr and b"one GPU only" in r.stderr and r.stdout == b""


def test_order_cli_refuses_index_on_stdin():
    r = subprocess.run([CLI, "build", "-s", "-i", "-", "-L", os.path.join(util.GOLDEN, "k2_fwd.txt")], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"not on stdin" in r.stderr and r.stdout == b""


@pytest.mark.parametrize("args", [["-2", "-s"], ["-s", "-2"], ["-r", "-2"]])
def test_order_cli_keeps_refusing_rb2(args):
    r = subprocess.run([CLI, "build"] + args + ["-L", os.path.join(util.GOLDEN, "k2_fwd.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"ropebwt2" in r.stderr


def test_order_usage_lists_s_and_r():
    r = subprocess.run([CLI, "build"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"-s          reverse lexicographic order" in r.stderr and b"-r          reverse-complement" in r.stderr
    assert b"Not available in this build (ropebwt2 insertion and debugging formats): -2 -T -e" in r.stderr
