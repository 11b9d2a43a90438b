"""tests/fmd_model.py -- the FMD data section restated in numpy -- pinned before test_gpu_fmd.py trusts it: against the reference's
own .fmd files (tests/golden), against the host writer (rb3h_fmdw_*, itself held to the reference library by
test_fmd_writer_wide_block_headers_vs_reference_library) on long runs with 32- and 64-bit block headers and on every run list of
tests/fmd_cases.py, and -- for the four BWTs of 10^8 runs whose .fmd meets the border of a superblock of 2^20 blocks -- against
`plain2fmd` of the host CLI, of the reference binary (where oracle/_ref is built) and the md5s tools/make_golden_fmdedge.py
recorded from it.  No GPU needed."""
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import fmd_cases as C
from tests import fmd_model as M
from tests import util

MAN = json.load(open(os.path.join(util.GOLDEN, "MANIFEST.json")))
EDGE = json.load(open(os.path.join(util.GOLDEN, "FMDEDGE_MANIFEST.json")))
CLI = _build.BIN_CLI


def _equal(got, want, ch=None):
    assert got.size == want.size and np.array_equal(got, want), M.describe(got, want, ch)


@pytest.mark.parametrize("name", sorted(k for k, v in MAN.items() if isinstance(v, dict) and "plain" in v and "fmd" in v))
def test_model_packs_and_unpacks_the_golden_files(name):
    ent = MAN[name]
    lut = np.full(256, 255, dtype=np.uint8)
    lut[np.frombuffer(b"$ACGTN", dtype=np.uint8)] = np.arange(6)
    plain = lut[np.frombuffer(gzip.open(os.path.join(util.GOLDEN, ent["plain"])).read().strip(), dtype=np.uint8)]
    assert plain.size == ent["n_symbols"] and int(plain.max()) <= 5
    lens, syms = M.runs_of_plain(plain)
    want, mcnt = C.fmd_data_words(np.fromfile(os.path.join(util.GOLDEN, ent["fmd"]), dtype=np.uint8))
    ch = M.chain(lens)
    _equal(M.pack(lens, syms, ch), want, ch)
    l2, s2 = M.unpack(want)
    assert np.array_equal(l2, lens) and np.array_equal(s2, syms)
    assert np.array_equal(C.sym_counts(lens, syms), mcnt)


def _wide_header_runs(case):
    """the run generators of test_fmd_writer_wide_block_headers_vs_reference_library (tests/test_cpu_host.py)"""
    rng = np.random.default_rng({"w32": 1, "w64": 2, "mixed": 3}[case])
    runs = []
    for i in range(400):
        if case == "w32":
            l = int(rng.choice([1, 3, 17, 300, 20000, 70000, 1 << 20, (1 << 29) + 5]))
        elif case == "w64":
            l = int(rng.choice([1, 2, (1 << 30) + 3, (1 << 31) + 1, 1 << 33, (1 << 40) + 12345, 9]))
        else:
            l = int(rng.choice([1, 1, 2, 5, 40, 1000, 16384, 16383, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 1 << 36]))
        c = int(rng.integers(0, 6))
        if runs and runs[-1][1] == c:
            c = (c + 1) % 6
        runs.append((l, c))
    return np.array([r[0] for r in runs], dtype=np.int64), np.array([r[1] for r in runs], dtype=np.uint8)


def _host_vs_model(lens, syms, tmp_path, ch=None):
    want, mcnt = C.fmd_data_words(np.fromfile(C.host_fmd_file(lens, syms, tmp_path / "host.fmd"), dtype=np.uint8))
    ch = M.chain(lens) if ch is None else ch
    _equal(M.pack(lens, syms, ch), want, ch)
    assert np.array_equal(C.sym_counts(lens, syms), mcnt)
    return want, ch


@pytest.mark.parametrize("case", ["w32", "w64", "mixed"])
def test_model_equals_host_writer_on_wide_headers(case, tmp_path):
    lens, syms = _wide_header_runs(case)
    want, ch = _host_vs_model(lens, syms, tmp_path)
    assert (1 in ch.type) if case == "w32" else (2 in ch.type), "the generator reaches the header width it is named after"
    l2, s2 = M.unpack(want)
    assert np.array_equal(l2, lens) and np.array_equal(s2, syms)


@pytest.mark.parametrize("name", C.SMALL)
def test_model_equals_host_writer_on_the_packer_cases(name, tmp_path):
    lens, syms = C.small(name)
    ch = M.chain(lens)
    C.check_small(name, lens, ch)
    want, _ = _host_vs_model(lens, syms, tmp_path, ch)
    if lens.size <= 40000:
        l2, s2 = M.unpack(want)
        assert np.array_equal(l2, lens) and np.array_equal(s2, syms)


@pytest.mark.parametrize("which", ["a", "b"])
def test_model_equals_host_writer_at_two_to_the_thirty(which, tmp_path):
    lens, syms = C.wide(which)
    ch = M.chain(lens)
    C.check_wide(which, lens, ch)
    want, _ = _host_vs_model(lens, syms, tmp_path, ch)
    l2, s2 = M.unpack(want)
    assert np.array_equal(l2, lens) and np.array_equal(s2, syms)   # (no run straddles a block: each block decodes on its own)
    t, cnt = M.header_counts(want, 1)
    assert t == ch.type[1] and cnt[0] == ch.n_sym[0] and cnt[1:] == C.sym_counts(lens[:13], syms[:13]).tolist()


def test_model_equals_host_writer_on_the_decoder_runs(tmp_path):
    lens, syms, marks = C.long_runs()
    C.check_long_runs(lens, marks)
    _host_vs_model(lens, syms, tmp_path)


def test_describe_names_the_block():
    lens, syms = C.small("P2b")
    ch = M.chain(lens)
    good = M.pack(lens, syms, ch)
    bad = good.copy()
    bad[8 + 5] ^= np.uint64(1 << 40)
    s = M.describe(bad, good, ch)
    assert "block 1 " in s and "word 5 (payload)" in s and "runs 20..32" in s and "type 1 against 1" in s, s
    assert M.describe(good, good) == "the streams agree"


@pytest.fixture(scope="module", params=sorted(C.SUPER))
def superblock(request, tmp_path_factory):
    """(case, chain, the model's words, path of the plain text, path of the host CLI's .fmd)"""
    case = request.param
    d = tmp_path_factory.mktemp("sb_" + case)
    src, out = str(d / "bwt.txt"), str(d / "host.fmd")
    plain = C.super_plain(case)
    np.frombuffer(b"$ACGTN", dtype=np.uint8)[plain].tofile(src)
    lens, syms = M.runs_of_plain(plain)
    assert np.array_equal(lens, C.super_lens(case))
    ch = M.chain(lens)
    C.check_super(case, ch)
    words = M.pack(lens, syms, ch)
    subprocess.run([CLI, "plain2fmd", "-o", out, src], check=True, stderr=subprocess.DEVNULL)
    yield case, ch, words, src, out
    os.remove(src), os.remove(out)


def test_superblock_host_plain2fmd_equals_model_and_manifest(superblock):
    case, ch, words, src, out = superblock
    ent = EDGE[case]
    got, mcnt = C.fmd_data_words(np.fromfile(out, dtype=np.uint8))
    assert words.size == ent["n_words"] == C.super_n_words(case, ch) and words.nbytes == ent["data_bytes"]
    assert int(mcnt.sum()) == ent["n_symbols"] and C.SUPER[case] == ent["n_runs"]
    assert hashlib.md5(words.tobytes()).hexdigest() == ent["data_md5"], "the model differs from what the reference wrote"
    _equal(got, words, ch)


def test_superblock_reference_plain2fmd_equals_host(superblock, tmp_path):
    case, ch, words, src, out = superblock
    if not os.path.exists(util.REF_BIN):
        pytest.skip("no reference binary")
    ref = str(tmp_path / "ref.fmd")
    subprocess.run([util.REF_BIN, "plain2fmd", "-o", ref, src], check=True, stderr=subprocess.DEVNULL)
    a, b = np.fromfile(ref, dtype=np.uint8), np.fromfile(out, dtype=np.uint8)
    _equal(C.fmd_data_words(a)[0], words, ch)
    assert a.size == b.size and np.array_equal(a, b), "the whole file: header, data section and rank index"
