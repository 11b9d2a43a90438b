#!/usr/bin/env python3
"""Golden answers of the reference's `kount` on the committed indexes: runs the unmodified reference binary (oracle/_ref/ropebwt3,
built by oracle/Makefile) on every case of CASES and records the arguments, the exit status, the number of output lines and the md5
of stdout in tests/golden/KOUNT_MANIFEST.json (data only; tests/test_gpu_kount.py compares the CLI with it).
    python tools/make_golden_kount.py"""
import hashlib, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "KOUNT_MANIFEST.json")


def cases():
    idx = sorted(f for f in os.listdir(GOLDEN) if f.endswith((".fmd", ".fmr")))
    for f in idx:                                          # every index alone
        for k in (1, 3, 31, 51, 80):
            for m in (1, 2, 100):
                yield ["-k%d" % k, "-m%d" % m, f]
    yield ["-k6", "-m0", "k2_fwd.fmd"]                     # all 4^k k-mers
    yield ["-k2", "-m-5", "edge_chars.fmd"]
    yield ["-k80", "-m3", "genomes12.fmd"]
    yield ["-k25", "-m2", "genomes12_first6.fmr", "reads_fq.fmd", "edge_chars.fmd"]   # several indexes, FMR with FMD
    yield ["-k31", "-m2", "genomes12_first6.fmd", "genomes12_first6.fmr"]
    yield ["-k17", "-m3", "reads_fwd.fmd", "reads_rev.fmd"]
    yield ["-k4", "-m1", "k4_readme.fmd", "k3_both.fmd", "k2_fwd.fmd"]
    yield ["-k12", "-m1000000000", "genomes12.fmd"]        # nothing occurs that often
    yield ["-k51", "-m2", "reads_fq.fmd"]
    yield ["-k31", "-m2", "genomes12.fmd"]


man = {}
t0 = time.time()
for args in cases():
    key = " ".join(args)
    if key in man:
        continue
    r = subprocess.run([ref, "kount"] + args[:2] + [os.path.join(GOLDEN, f) for f in args[2:]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    man[key] = {"args": args, "exit": r.returncode, "lines": r.stdout.count(b"\n"), "md5": hashlib.md5(r.stdout).hexdigest()}
print("%d cases in %.1f s" % (len(man), time.time() - t0), file=sys.stderr)
json.dump(man, open(man_fn, "w"), indent=1, sort_keys=True)
open(man_fn, "a").write("\n")
