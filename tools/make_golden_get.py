#!/usr/bin/env python3
"""Golden answers of the reference's `get` on the committed indexes: runs the unmodified reference binary (oracle/_ref/ropebwt3, built
by oracle/Makefile) on every case and records the arguments as typed ("args": the index by its name under tests/golden, "index" says
which one it is), the rows the command answers ("rows": the arguments behind the index through atol, those that begin with `-` left
out as the reference's option loop leaves them out), acc[1] and acc[6] of the index, the number of output lines and the md5 of stdout
in tests/golden/GET_MANIFEST.json -- and stdout itself where it is at most 4 kB (data only; tests/test_gpu_get.py compares the CLI
with it, tests/test_cpu_get.py checks what the manifest must hold and restates the walk).
    python tools/make_golden_get.py"""
import hashlib, json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ropebwt3_amd import _build
from tests import kount_model as km
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "GET_MANIFEST.json")

INDEXES = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
           "edge_dups.fmd", "longruns.fmd", "copies3000.fmd", "reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"]
TEXT_MAX = 4096
ACC = {}


def acc_of(idx):
    if idx not in ACC:
        b = km.golden_plain(GOLDEN, idx, _build.BIN_CLI)
        ACC[idx] = [0] + [int(x) for x in np.cumsum(np.bincount(b, minlength=6))]
    return ACC[idx]


def atol(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def cases():
    for idx in INDEXES:
        a = acc_of(idx)
        yield [idx] + [str(x) for x in (0, 1, a[1] - 1, a[1], a[6] - 1, a[6])], idx    # sentinel rows, a row inside a string, the last row, one too many
        yield ["-1", idx, "0", "abc", "1", "1", str(a[6] + 7), "3x"], idx              # a swallowed option, a word (row 0), a duplicate, out of range, digits then letters
    yield ["edge_dups.fmd"] + [str(x) for x in range(14)], "edge_dups.fmd"              # all 12 strings (duplicates, AA / NN) and two rows inside strings
    yield ["genomes12.fmd"] + [str(x) for x in range(24)], "genomes12.fmd"
    yield ["reads_fq.fmd"] + [str(x) for x in range(6104)], "reads_fq.fmd"              # many more rows than a block has octets
    yield ["longruns.fmd"] + [str(x) for x in range(8)], "longruns.fmd"                 # the longest serial chains here
    yield ["copies3000.fmd"] + [str(x) for x in range(100)], "copies3000.fmd"
    yield ["genomes12_first6.fmr"] + [str(x) for x in range(12)], "genomes12_first6.fmr"
    yield ["-1", "k3_both.fmd", "0", "1", "5", "99999", "abc", "7"], "k3_both.fmd"


man = {}
t0 = time.time()
for args, idx in cases():
    key = " ".join(args) if len(args) <= 16 else " ".join(args[:3]) + " .. " + args[-1]
    r = subprocess.run([ref, "get"] + [os.path.join(GOLDEN, x) if x == idx else x for x in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0:
        sys.exit("the reference failed on %s" % key)
    a = acc_of(idx)
    rows = [atol(x) for x in args[args.index(idx) + 1:] if not x.startswith("-")]
    e = {"args": args, "index": idx, "rows": rows, "acc1": a[1], "acc6": a[6], "lines": r.stdout.count(b"\n"), "md5": hashlib.md5(r.stdout).hexdigest()}
    if len(r.stdout) <= TEXT_MAX:
        e["stdout"] = r.stdout.decode("latin-1")
    assert key not in man, key
    man[key] = e
print("%d cases in %.1f s; %d with their text" % (len(man), time.time() - t0, sum(1 for e in man.values() if "stdout" in e)), file=sys.stderr)
json.dump(man, open(man_fn, "w"), indent=0, sort_keys=True)
open(man_fn, "a").write("\n")
