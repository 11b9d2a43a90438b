"""build -s / -r on the GPU: the string order kernel and the sentinel ranks against the Python model, merges in a sorted
order against the CPU oracle, and the CLI against the reference binary byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from ropebwt3_amd.gpu import SO_RLO, SO_RCLO, SO_IO, Rb3GpuError
from tests import util
from tests import order_model as om

CLI = _build.BIN_CLI
SOS = [SO_RLO, SO_RCLO]


def _reads_collection(rng, n=3000):
    g = util.random_genome(rng, 20000)
    out = []
    for _ in range(n):
        L = int(rng.integers(1, 301))
        s = int(rng.integers(0, len(g) - L))
        r = g[s:s + L].copy()
        r[rng.random(L) < 0.01] = 5
        out.append(r)
    out += [out[i].copy() for i in rng.integers(0, len(out), size=300)]          # duplicates
    out += [out[i][int(rng.integers(len(out[i]))):].copy() for i in rng.integers(0, len(out), size=200)]  # suffixes
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("so", SOS)
def test_order_strings_matches_python(engine, so):
    rng = np.random.default_rng(so)
    strings = _reads_collection(rng)
    tail = util.random_genome(rng, 10000)
    strings += [np.concatenate([util.random_genome(rng, 10000), tail]) for _ in range(4)]   # 20 kb strings sharing 10 kb tails
    strings += [tail.copy(), np.concatenate([tail[:5], tail])]
    text = util.make_text(strings)
    got = engine.order_strings(text, so)
    assert np.array_equal(got, om.ordered_text(text, so))


@pytest.mark.gpu
@pytest.mark.parametrize("so", SOS)
def test_sentinel_ranks_match_python(oracle, so):
    from ropebwt3_amd import Rb3Gpu
    rng = np.random.default_rng(10 + so)
    old, new = _reads_collection(rng, 1500), _reads_collection(rng, 800)
    old_t = om.ordered_text(util.make_text(old), so)
    new_t = om.ordered_text(util.make_text(new), so)
    h = Rb3Gpu(verbose=1)
    try:
        h.set_order(so)
        assert h.get_order() == so
        h.from_plain(oracle.bwt(old_t))
        d_bwt, d_tw = h.sort_text(new_t)
        want = om.p0(om.strings_of(old_t), om.strings_of(new_t), so)
        m = len(want)
        for tw in (d_tw, None):   # text-order words, or the batch's own BWT
            p0 = h.sentinel_ranks_dev(d_bwt, tw, new_t.size, m)
            assert np.all(np.diff(p0) >= 0)
            assert np.array_equal(p0, want)
        with pytest.raises(Rb3GpuError):   # a wrong string count
            h.sentinel_ranks_dev(d_bwt, d_tw, new_t.size, m + 1)
        # a batch that is NOT in the order: p0 decreases somewhere, and the merge says so instead of building a wrong index
        rev_t = om.text_of(om.ordered(om.strings_of(new_t), so)[::-1])
        d_b3 = h.dev_upload(oracle.bwt(rev_t))
        with pytest.raises(Rb3GpuError) as e:
            h.sentinel_ranks_dev(d_b3, None, rev_t.size, m)
        assert e.value.code == -6
        before = h.export_plain()
        with pytest.raises(Rb3GpuError):
            h.merge_plain_dev(d_b3, rev_t.size)
        assert np.array_equal(h.export_plain(), before)
        for p in (d_bwt, d_tw, d_b3):
            h.dev_free(p)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("so", SOS)
@pytest.mark.parametrize("path", ["text", "text_sa", "plain", "plain_host", "step"])
def test_merge_in_order_matches_oracle(oracle, so, path):
    from ropebwt3_amd import Rb3Gpu
    rng = np.random.default_rng(20 + so)
    if path == "step":   # long strings: walkers inside the strings (merge_text_step_dev)
        g = util.random_genome(rng, 60000)
        old = [util.mutate(rng, g, 0.002) for _ in range(4)] + [g[:30000]]
        new = [util.mutate(rng, g, 0.002) for _ in range(3)] + [g.copy(), g[10000:]]
    else:
        old, new = _reads_collection(rng, 2000), _reads_collection(rng, 1500)
    h = Rb3Gpu(verbose=1)
    try:
        h.set_order(so)
        first = h.bwt_from_text(util.make_text(old))[0]   # the handle orders the text before it sorts it
        h.from_plain_dev(first, util.make_text(old).size)
        h.dev_free(first)
        assert np.array_equal(h.export_plain(), oracle.bwt(om.ordered_text(util.make_text(old), so)))
        t = util.make_text(new)
        m = int((t == 0).sum())
        if path in ("text", "text_sa", "step"):
            d_bwt, d_tw, d_sa = h.sort_text_sa(t)
            if path == "text":
                h.merge_text_dev(d_bwt, d_tw, t.size, m)
            elif path == "text_sa":
                h.merge_text_dev(d_bwt, d_tw, t.size, m, d_sa=d_sa)
            else:
                h.merge_text_step_dev(d_bwt, d_tw, t.size, m, 512, d_sa=d_sa)
            for p in (d_bwt, d_tw, d_sa):
                h.dev_free(p)
        else:
            b2 = oracle.bwt(om.ordered_text(t, so))
            if path == "plain":
                d = h.dev_upload(b2)
                h.merge_plain_dev(d, b2.size)
                h.dev_free(d)
            else:
                h.merge_plain(b2)
        want = oracle.bwt(om.ordered_text(util.make_text(old + new), so))
        assert np.array_equal(h.export_plain(), want)
        assert h.stats()["n_fallbacks"] == 0
    finally:
        h.close()


@pytest.mark.gpu
def test_order_input_order_only_entry_points(oracle):
    """the stages of a multi-GPU merge and the whole-index merge walk in input order only: they say so"""
    from ropebwt3_amd import Rb3Gpu
    h, g = Rb3Gpu(verbose=0), Rb3Gpu(verbose=0)
    try:
        b = oracle.bwt(util.make_text([util.random_genome(np.random.default_rng(1), 500)]))
        h.from_plain(b)
        g.from_plain(b)
        h.set_order(SO_RLO)
        d = h.dev_upload(b)
        with pytest.raises(Rb3GpuError) as e:
            h.mg_begin(d, b.size)
        assert e.value.code == -7
        with pytest.raises(Rb3GpuError) as e:
            h.merge_index(g)
        assert e.value.code == -7
        h.dev_free(d)
        h.set_order(SO_IO)
        assert h.get_order() == SO_IO
    finally:
        h.close()
        g.close()


# ---- the CLI against the reference -------------------------------------------------------------------------

def _ref(args):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    r = subprocess.run([util.REF_BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


def _ours(args):
    r = subprocess.run([CLI, "build"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    return r.stdout, r.stderr


def _fmr_plain(data, tmp_path, tag):
    p = tmp_path / ("%s.fmr" % tag)
    p.write_bytes(data)
    out, _ = _ours(["-i", str(p)])   # no input files: the index as plain text
    return out


G = lambda f: os.path.join(util.GOLDEN, f)   # noqa: E731
CASES = {
    "reads_fq": [G("reads_fq.fa.gz")],
    "reads_fwd": ["-L", "-R", G("reads_fwd.txt.gz")],
    "reads_rev": ["-L", "-F", G("reads_rev.txt.gz")],
    "copies3000": ["-L", G("copies3000.txt.gz")],
    "edge_chars": ["-L", G("edge_chars.txt")],
    "edge_dups": ["-L", G("edge_dups.txt")],
    "genomes12": [G("genomes12.fa.gz")],
}


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["-s", "-r"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cli_order_matches_reference(tmp_path, name, opt):
    args = CASES[name]
    for fmt in ([], ["-d"]):
        got, _ = _ours([opt] + fmt + args)
        assert got == _ref(["build", opt] + fmt + args), (name, opt, fmt)
    got, _ = _ours([opt, "-b"] + args)
    want = _ref(["build", opt, "-b"] + args)
    assert got[:4] == want[:4] == b"RB\2" + bytes([1 if opt == "-s" else 2])
    assert _fmr_plain(got, tmp_path, "g") == _fmr_plain(want, tmp_path, "w")


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["-s", "-r"])
@pytest.mark.parametrize("extra,name", [
    (["-m", "400k"], "copies3000"),
    (["--gpu-batch", "100k"], "reads_fq"),
    (["--gpu-batch", "100k", "-p", "3", "-t", "2"], "genomes12"),   # (-t <= -p: the order holds in the reference too)
    (["-m", "45k"], "genomes12"),
    (["--gpu-batch", "30k"], "reads_fwd"),
])
def test_cli_order_batches(name, opt, extra):
    """sub-batches and batches: each is ordered on its own and merged in the order (the result depends only on the multiset)"""
    args = CASES[name]
    got, _ = _ours([opt, "-d"] + extra + args)
    ref_extra = [a for i, a in enumerate(extra) if a != "--gpu-batch" and (i == 0 or extra[i - 1] != "--gpu-batch")]
    assert got == _ref(["build", opt, "-d"] + ref_extra + args)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["-s", "-r"])
def test_cli_order_files_rebatch_checkpoint(tmp_path, opt):
    parts = [G("genomes12_part%d.fa.gz" % i) for i in range(3)]
    want = _ref(["build", opt, "-d"] + parts)
    got, _ = _ours([opt, "-d"] + parts)
    assert got == want
    got, _ = _ours([opt, "-d", "--rebatch", "--gpu-batch", "100k"] + parts)
    assert got == want
    ck = tmp_path / "ck.fmr"
    got, _ = _ours([opt, "-d", "-S", str(ck)] + parts)
    assert got == want and ck.read_bytes()[:4] == b"RB\2" + bytes([1 if opt == "-s" else 2])
    assert _fmr_plain(ck.read_bytes(), tmp_path, "ck") == _ref(["build", opt] + parts)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["-s", "-r"])
def test_cli_order_incremental(tmp_path, opt):
    """-i of an FMR made in an order (its header decides), of an FMD (input order), and the -p quirk (input order)"""
    first, rest = G("genomes12_first6.fa.gz"), G("genomes12_rest6.fa.gz")
    reads = G("reads_fq.fa.gz")
    fmr = tmp_path / "a.fmr"
    fmr.write_bytes(_ref(["build", opt, "-b", reads]))
    other = "-r" if opt == "-s" else "-s"
    for o in (opt, other):
        got, _ = _ours([o, "-d", "-i", str(fmr), first])
        assert got == _ref(["build", o, "-d", "-i", str(fmr), first])
    fmd = tmp_path / "a.fmd"
    fmd.write_bytes(_ref(["build", "-d", first]))
    got, _ = _ours([opt, "-d", "-i", str(fmd), rest])
    assert got == _ref(["build", opt, "-d", "-i", str(fmd), rest])
    got, _ = _ours([opt, "-d", "-p1", "-t4", reads])
    assert got == _ref(["build", opt, "-d", "-p1", "-t4", reads])


@pytest.mark.gpu
def test_cli_order_reads_m7g_at_scale(tmp_path):
    """build -L -r -d -m7g on the 10 M reads of tools/gen_reads.py (3.02 G symbols: six GPU sub-batches, each ordered on the device, five
    ordered merges): the md5 the reference records in ORDER_MANIFEST.json (tools/make_golden_order.py)"""
    import hashlib
    import json
    from tools import gen_reads
    ent = json.load(open(os.path.join(util.GOLDEN, "ORDER_MANIFEST.json")))["reads_m7g_rclo"]
    fn = gen_reads.generate(ent["n_reads"], str(tmp_path / "reads.txt"))
    out = tmp_path / "out.fmd"
    r = subprocess.run([CLI, "build"] + ent["flags"] + ["-o", str(out), fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    data = out.read_bytes()
    assert len(data) == ent["fmd_bytes"] and hashlib.md5(data).hexdigest() == ent["fmd_md5"]
