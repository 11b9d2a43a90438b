"""BRE on the GPU: rb3gpu_export_bre / rb3gpu_from_bre / rb3gpu_merge_bre against the Python model (tests/bre_model.py), `build -e`
against the files the unmodified reference wrote (tests/golden/BRE_MANIFEST.json, *.bre), and every index-reading command on a
.bre against the same command on the .fmd."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ropebwt3_amd import Rb3Gpu, Rb3GpuError, _build, gpu
from tests import bre_model, util
from tests.test_cpu_bre import BROKEN, FIXTURES, PLAIN, plain_bwt

pytestmark = pytest.mark.gpu

CLI = _build.BIN_CLI
GOLDEN = util.GOLDEN
MAN = json.load(open(os.path.join(GOLDEN, "BRE_MANIFEST.json")))
BUILD = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
COUNTS = ("n_rec", "n_sym", "n_run")


def g(name):
    return os.path.join(GOLDEN, name)


def cli(args, env=None):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=None if env is None else dict(os.environ, **env))


def ok(args, env=None):
    r = cli(args, env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-800:]
    return r.stdout


def fixture_runs(name):
    if name in PLAIN:
        return bre_model.runs_of(plain_bwt(name))
    return bre_model.decode(open(g(name + ".bre"), "rb").read())[1]


@pytest.fixture(scope="module")
def h():
    e = Rb3Gpu(device=0, verbose=1)
    yield e
    e.close()


# ---- export ----

def edge_runs():
    """runs of max - 1, max, max + 1, 2 max, 2 max + 1 for one and two length bytes, one of 1 000 000, one that ends on a group
    boundary (8192 symbols) exactly, one that crosses the next, and a few thousand short ones"""
    runs, c = [(0, 3)], 0
    for mx in (255, 65535):
        for l in (mx - 1, mx, mx + 1, 2 * mx, 2 * mx + 1):
            c = c % 5 + 1
            runs.append((c, l))
    c = c % 5 + 1
    runs.append((c, 1000000))
    pos = sum(l for _, l in runs)
    c = c % 5 + 1
    runs.append((c, 8192 - pos % 8192 + 8192))   # ends on a boundary
    c = c % 5 + 1
    runs.append((c, 100))
    c = c % 5 + 1
    runs.append((c, 8192))                        # crosses the next one
    rng = np.random.default_rng(7)
    for l in rng.integers(1, 9, size=3000):
        c = c % 5 + 1
        runs.append((c, int(l)))
    assert sum(l for _, l in runs[:-3002]) % 8192 == 0
    return runs


@pytest.fixture(scope="module")
def edge(h):
    runs = edge_runs()
    return runs, bre_model.plain_of(runs)


@pytest.mark.parametrize("bpr", [1, 2, 3, 4])
def test_export_edges(h, edge, bpr):
    runs, plain = edge
    h.from_plain(plain)
    want, counts = bre_model.records(runs, bpr)
    if bpr == 1:
        assert -(-1000000 // 255) == 3922
    st = {}
    got = h.export_bre(bpr, st)
    print(bpr, len(got), st)
    assert tuple(st[k] for k in COUNTS) == counts and st["n_pieces"] == 1
    assert got == want


@pytest.mark.parametrize("name", ["reads_fq", "longruns", "edges"])
def test_export_in_pieces(h, edge, name):
    runs = edge[0] if name == "edges" else fixture_runs(name)
    h.from_plain(edge[1] if name == "edges" else bre_model.plain_of(runs))
    try:
        for bpr in (1, 2, 3, 4):
            want, counts = bre_model.records(runs, bpr)
            for piece in (0, 32768, 1):
                h.tune("bre_piece", piece)
                st = {}
                got = h.export_bre(bpr, st)
                print(name, bpr, piece, st["n_pieces"])
                assert got == want, (bpr, piece)
                assert tuple(st[k] for k in COUNTS) == counts
                if piece == 1 or (piece and counts[2] > 2 * 32768):
                    assert st["n_pieces"] > 1
                if piece == 0:
                    assert st["n_pieces"] == 1
    finally:
        h.tune("bre_piece", 0)


def test_export_arguments(h, edge):
    h.from_plain(edge[1][:1000])
    for bpr in (0, 5, 8, -1):
        with pytest.raises(Rb3GpuError):
            h.export_bre(bpr)


# ---- import ----

@pytest.mark.parametrize("chunk", [0, 1])
@pytest.mark.parametrize("name", PLAIN + ["longruns"])
def test_from_bre(h, name, chunk):
    runs = fixture_runs(name)
    plain = bre_model.plain_of(runs)
    acc = np.concatenate(([0], np.cumsum(np.bincount(plain, minlength=6))))
    if chunk:
        h.tune("load_chunk", chunk)
    try:
        for bpr in (1, 2, 4, 8):
            for joined in (True, False):
                rec, counts = bre_model.records(runs, bpr, joined)
                st = {}
                h.from_bre(rec, bpr, st)
                assert tuple(st[k] for k in COUNTS) == counts, (bpr, joined)
                assert st["n_pieces"] == (1 if not chunk or plain.size <= 8192 else plain.size // 8192 + 1)
                assert np.array_equal(h.export_plain(), plain), (bpr, joined)
                assert list(h.get_acc()) == list(acc)
    finally:
        h.tune("load_chunk", 16384)


def test_from_bre_refuses(h):
    rec, _ = bre_model.records(fixture_runs("k4_readme"), 2)
    for bad in (rec[:9] + b"\x06" + rec[10:], rec[:10] + b"\0\0" + rec[12:]):   # a symbol above 5, a record of no symbols
        with pytest.raises(Rb3GpuError) as e:
            h.from_bre(bad, 2)
        assert e.value.code == -4   # RB3GPU_ESYMBOL
    with pytest.raises(Rb3GpuError) as e:
        h.from_bre(b"\x01" + (1 << 56).to_bytes(8, "little"), 8)   # 2^56 symbols in one record
    assert e.value.code == -4
    for bpr, r in ((0, rec), (9, bytes(20)), (2, b"")):
        with pytest.raises(Rb3GpuError) as e:
            h.from_bre(r, bpr)
        assert e.value.code == -3   # RB3GPU_EINVAL
        with pytest.raises(Rb3GpuError) as e:
            h.merge_bre(r, bpr)
        assert e.value.code == -3


def test_merge_bre(h, tmp_path):
    first = ok(["build", "-e", "-i", g("genomes12_first6.fmd")])
    rest = ok(["build", "-e", g("genomes12_rest6.fa.gz")])
    (tmp_path / "a.bre").write_bytes(first)
    (tmp_path / "b.bre").write_bytes(rest)
    bpr_a, rec_a, _ = gpu.read_bre(str(tmp_path / "a.bre"))
    bpr_b, rec_b, cnt_b = gpu.read_bre(str(tmp_path / "b.bre"))
    rest_plain = bre_model.plain_of(bre_model.decode(rest)[1])
    h.from_bre(rec_a, bpr_a)
    st = {}
    h.merge_bre(rec_b, bpr_b, st)
    assert tuple(st[k] for k in COUNTS) == cnt_b
    got = h.export_plain()
    h2 = Rb3Gpu(device=0, verbose=1)
    h2.from_plain(bre_model.plain_of(bre_model.decode(first)[1]))
    h2.merge_plain(rest_plain)
    want = h2.export_plain()
    h2.close()
    assert np.array_equal(got, want) and np.array_equal(got, plain_bwt("genomes12"))


# ---- `build -e` ----

@pytest.mark.parametrize("name", sorted(MAN["from_fmd"]))
def test_cli_build_e_from_index(name):
    ent = MAN["from_fmd"][name]
    out = ok(["build", "-e", "-i", g(name + ".fmd")])
    assert len(out) == ent["bytes"] and hashlib.md5(out).hexdigest() == ent["md5"]
    if "file" in ent:
        assert out == open(g(ent["file"]), "rb").read()
    assert ok(["build", "-e", "--host-fmd", "-i", g(name + ".fmd")]) == out
    runs = bre_model.decode(out)[1]
    assert ok(["build", "-e", "--bre-run-bytes", "1", "-i", g(name + ".fmd")]) == bre_model.encode(runs, 1)


@pytest.mark.parametrize("key", sorted(MAN["from_seq"]))
def test_cli_build_e_from_sequences(key):
    ent = MAN["from_seq"][key]
    for extra in ([], ["-m100k"]):
        out = ok(["build", "-e"] + ent["flags"] + extra + [g(ent["input"])])
        assert len(out) == ent["bytes"] and hashlib.md5(out).hexdigest() == ent["md5"], extra


def test_cli_build_e_options(tmp_path):
    ent = MAN["from_fmd"]["genomes12"]
    r = cli(["build", "-e", "-o", str(tmp_path / "o.bre"), "-i", g("genomes12.fmd")])
    assert r.returncode == 0 and r.stdout == b"" and hashlib.md5((tmp_path / "o.bre").read_bytes()).hexdigest() == ent["md5"]
    files = [g(p) for p in BUILD["genomes12_files"]["inputs"]]
    for extra in (["--gpus", "2"], ["--gpus", "2", "--interval", "-m100k"]):
        assert hashlib.md5(ok(["build", "-e"] + extra + files)).hexdigest() == ent["md5"], extra
    for bpr in ("3", "4"):
        out = ok(["build", "-e", "--bre-run-bytes", bpr, "-i", g("longruns.fmd")])
        assert out == bre_model.encode(fixture_runs("longruns"), int(bpr))
    for bad in ("0", "5"):
        r = cli(["build", "-e", "--bre-run-bytes", bad, "-i", g("k4_readme.fmd")])
        assert r.returncode == 1 and r.stdout == b""
    r = cli(["build", "-T", "-i", g("k4_readme.fmd")])
    assert r.returncode == 1 and r.stdout == b"" and b"output format -T is not available" in r.stderr
    assert b"-e " in cli(["build"]).stderr


# ---- reading ----

READ = ["genomes12", "longruns", "copies3000", "k2_fwd"]


@pytest.fixture(scope="module")
def placed(tmp_path_factory):
    """name -> (x.fmd, x.bre) in one directory, the .bre written by the model, each with the same .ssa (made by `ssa -s8`) and .len.gz beside it"""
    root = tmp_path_factory.mktemp("bre")
    done = {}

    def get(name):
        if name not in done:
            fmd, bre = str(root / (name + ".fmd")), str(root / (name + ".bre"))
            shutil.copy(g(name + ".fmd"), fmd)
            open(bre, "wb").write(bre_model.encode(fixture_runs(name), 2))
            ok(["ssa", "-s8", "-o", fmd + ".ssa", fmd])
            shutil.copy(fmd + ".ssa", bre + ".ssa")
            if os.path.exists(g(name + ".len.gz")):
                shutil.copy(g(name + ".len.gz"), fmd + ".len.gz")
                shutil.copy(g(name + ".len.gz"), bre + ".len.gz")
            done[name] = (fmd, bre)
        return done[name]
    return get


Q, QSW = g("mem_mutated.fa.gz"), g("sw_reads.fa")
COMMANDS = {
    "build -d -i": lambda x: ["build", "-d", "-i", x],
    "build -b -i": lambda x: ["build", "-b", "-i", x],
    "merge first6.fmr x": lambda x: ["merge", "-d", g("genomes12_first6.fmr"), x],
    "merge x other.fmd": lambda x: ["merge", x, g("k4_readme.fmd")],
    "ssa -s8": lambda x: ["ssa", "-s8", x],
    "kount": lambda x: ["kount", "-k31", "-m2", x],
    "mem -l19": lambda x: ["mem", "-l19", x, Q],
    "mem -l31 -p10": lambda x: ["mem", "-l31", "-p10", x, Q],
    "suffix": lambda x: ["suffix", x, Q],
    "get": lambda x: ["get", x, "0", "1", "2"],
    "hapdiv": lambda x: ["hapdiv", x, Q],
    "sw -e -p3": lambda x: ["sw", "-e", "-p3", x, QSW],
    "sw --local": lambda x: ["sw", "--local", x, QSW],
    "build -i x more": lambda x: ["build", "-d", "-i", x, g("genomes12_rest6.fa.gz")],
    "recode": lambda x: ["recode", "-d", x],
    "build -d --host-fmd -i": lambda x: ["build", "-d", "--host-fmd", "-i", x],
}


BOTH_STRANDS = ("mem -l19", "mem -l31 -p10", "hapdiv", "sw -e -p3", "sw --local")   # refused on k2_fwd, which holds one strand (and has no .len.gz)


@pytest.mark.parametrize("cmd", sorted(COMMANDS))
@pytest.mark.parametrize("name", READ)
def test_cli_reads_bre_like_fmd(placed, name, cmd):
    if name == "k2_fwd" and cmd in BOTH_STRANDS:
        return   # (nothing to compare: the command cannot work on this index in any format)
    fmd, bre = placed(name)
    a, b = cli(COMMANDS[cmd](fmd)), cli(COMMANDS[cmd](bre))
    print(name, cmd, a.returncode, len(a.stdout))
    assert (b.returncode, b.stdout) == (a.returncode, a.stdout), b.stderr.decode(errors="replace")[-600:]
    assert a.returncode == 0, a.stderr.decode(errors="replace")[-600:]
    if name == "genomes12" or cmd in ("build -d -i", "build -b -i", "ssa -s8", "get", "recode"):
        assert len(a.stdout) > 0
    if cmd == "build -d -i":
        assert b.stdout == open(g(name + ".fmd"), "rb").read()


def test_cli_reads_other_run_bytes_and_chunks(placed, tmp_path):
    want = open(g("genomes12.fmd"), "rb").read()
    runs = fixture_runs("genomes12")
    for bpr, joined in ((1, True), (4, False), (8, True)):
        p = tmp_path / ("g%d.bre" % bpr)
        p.write_bytes(bre_model.encode(runs, bpr, joined, aux=b"xyz"))
        assert ok(["build", "-d", "-i", str(p)]) == want
        assert ok(["build", "-d", "-i", str(p)], env={"RB3GPU_LOAD_CHUNK": "3"}) == want


def test_cross_check_with_the_reference(tmp_path):
    if not os.path.exists(util.REF_BIN):
        pytest.skip("reference binary not built (oracle/_ref)")
    want = open(g("genomes12.fmd"), "rb").read()
    for bpr in ("1", "2", "4"):
        p = str(tmp_path / ("ours%s.bre" % bpr))
        ok(["build", "-e", "--bre-run-bytes", bpr, "-o", p, "-i", g("genomes12.fmd")])
        r = subprocess.run([util.REF_BIN, "build", "-d", "-i", p], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == want
    p = str(tmp_path / "ref.bre")
    subprocess.run([util.REF_BIN, "build", "-e", "-o", p, "-i", g("genomes12.fmd")], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert hashlib.md5(open(p, "rb").read()).hexdigest() == MAN["from_fmd"]["genomes12"]["md5"]
    assert ok(["build", "-d", "-i", p]) == want


@pytest.mark.parametrize("what", sorted(BROKEN))
def test_cli_refusals(what, tmp_path):
    p = tmp_path / "bad.bre"
    p.write_bytes(BROKEN[what])
    for args in (["build", "-d", "-i", str(p)], ["kount", "-k5", str(p)], ["merge", g("k4_readme.fmd"), str(p)]):
        r = cli(args)
        assert r.returncode == 1 and r.stdout == b"", (args, r.stderr)
        assert stderr_is_one_line(r, args), r.stderr


def stderr_is_one_line(r, args):
    """one ERROR line and nothing else -- for merge, beside the two lines with which the engine has reported the loading of the base index before"""
    lines = r.stderr.decode().strip().splitlines()
    if args[0] == "merge":
        lines = [l for l in lines if not l.startswith(("[M::fmd_words_to_b2::", "[M::rb3gpu_from_plain_dev::"))]
    return len(lines) == 1 and lines[0].startswith("ERROR")


def test_cli_refuses_a_footer_wrong_in_runs_only(tmp_path):
    """n_rec and n_sym agree and the host reader lets the file through: the device's run count is what catches it"""
    good = bre_model.encode(fixture_runs("genomes12"), 2)
    n_run = int.from_bytes(good[-8:], "little")
    p = tmp_path / "runs.bre"
    for delta in (1, -1):
        p.write_bytes(good[:-8] + (n_run + delta).to_bytes(8, "little"))
        assert gpu.read_bre(str(p))[2][2] == n_run + delta
        for args in (["build", "-d", "-i", str(p)], ["merge", g("k4_readme.fmd"), str(p)]):
            r = cli(args)
            assert r.returncode == 1 and r.stdout == b"" and stderr_is_one_line(r, args), r.stderr
    p.write_bytes(good)
    assert ok(["build", "-d", "-i", str(p)]) == open(g("genomes12.fmd"), "rb").read()


# ---- one open per index file: stdin and pipes ----

@pytest.fixture(scope="module")
def three_kinds(tmp_path_factory):
    """genomes12_first6 and genomes12_rest6 as .fmd, .fmr and .bre"""
    root = tmp_path_factory.mktemp("kinds")
    out = {}
    for name, src in (("first6", ["-i", g("genomes12_first6.fmd")]), ("rest6", [g("genomes12_rest6.fa.gz")])):
        for ext, flag in (("fmd", "-d"), ("fmr", "-b"), ("bre", "-e")):
            out[name, ext] = str(root / ("%s.%s" % (name, ext)))
            ok(["build", flag, "-o", out[name, ext]] + src)
    return out


@pytest.mark.parametrize("ext", ["fmd", "fmr", "bre"])
def test_merge_and_load_from_stdin(three_kinds, ext):
    want = open(g("genomes12.fmd"), "rb").read()
    data = open(three_kinds["rest6", ext], "rb").read()
    r = subprocess.run([CLI, "merge", "-d", g("genomes12_first6.fmr"), "-"], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode(errors="replace")[-600:]
    base = open(three_kinds["first6", ext], "rb").read()
    for args in (["merge", "-d", "-", three_kinds["rest6", "fmd"]], ["build", "-d", "-i", "-", g("genomes12_rest6.fa.gz")]):
        r = subprocess.run([CLI] + args, input=base, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and r.stdout == want, (args, r.stderr.decode(errors="replace")[-600:])


@pytest.mark.parametrize("ext", ["fmd", "fmr", "bre"])
def test_index_from_a_named_pipe(three_kinds, ext, tmp_path):
    """a pipe can be opened once: the magic is read in the one open that reads the rest"""
    import threading
    data = open(three_kinds["first6", ext], "rb").read()
    want = open(g("genomes12_first6.fmd"), "rb").read()
    merged = open(g("genomes12.fmd"), "rb").read()
    for n, (args, expect) in enumerate(((["build", "-d", "-i", None], want), (["merge", "-d", g("genomes12_first6.fmr"), None], None), (["merge", "-d", None, three_kinds["rest6", ext]], merged))):
        fifo = str(tmp_path / ("p%d" % n))
        os.mkfifo(fifo)
        payload = open(three_kinds["rest6", ext], "rb").read() if expect is None else data

        def feed():
            with open(fifo, "wb") as f:
                f.write(payload)
        t = threading.Thread(target=feed, daemon=True)
        t.start()
        r = cli([fifo if a is None else a for a in args])
        t.join(10)
        assert r.returncode == 0 and r.stdout == (merged if expect is None else expect), (args, r.stderr.decode(errors="replace")[-600:])
