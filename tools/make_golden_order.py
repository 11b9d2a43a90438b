#!/usr/bin/env python3
"""Golden md5 of the reference's .fmd for `build -L -r -d -m7g` (RCLO) on the N reads of tools/gen_reads.py: runs the unmodified
reference binary (oracle/_ref/ropebwt3, built by oracle/Makefile) once and records md5, size and its timing in
tests/golden/ORDER_MANIFEST.json under "reads_m7g_rclo".  N = 10,000,000 (3.02 G symbols) takes ~3 minutes on 8 cores.
    python tools/make_golden_order.py 10000000"""
import hashlib, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_reads
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(ROOT, "tests", "golden", "ORDER_MANIFEST.json")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000000
man = json.load(open(man_fn)) if os.path.exists(man_fn) else {}
flags = ["-L", "-r", "-d", "-m7g"]
threads = os.cpu_count() or 8
with tempfile.TemporaryDirectory() as d:
    fn = gen_reads.generate(N, os.path.join(d, "reads.txt"))
    t = time.time()
    r = subprocess.run([ref, "build"] + flags + ["-t%d" % threads, fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    dt = time.time() - t
man["reads_m7g_rclo"] = {"generator": "tools/gen_reads.py", "n_reads": N, "read_len": 150, "n_symbols": N * 302, "flags": flags,
                         "fmd_md5": hashlib.md5(r.stdout).hexdigest(), "fmd_bytes": len(r.stdout),
                         "reference_seconds": round(dt, 1), "reference_threads": threads,
                         "note": "oracle/_ref/ropebwt3 build -L -r -d -m7g (ropebwt2 insertion in RCLO order, one batch)"}
print(man["reads_m7g_rclo"], flush=True)
json.dump(man, open(man_fn, "w"), indent=1, sort_keys=True)
open(man_fn, "a").write("\n")
