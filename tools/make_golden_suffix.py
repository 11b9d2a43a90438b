#!/usr/bin/env python3
"""Golden answers of the reference's `suffix` on the committed indexes and query files: runs the unmodified reference binary
(oracle/_ref/ropebwt3, built by oracle/Makefile) on every case and records the options, the files (index first; names under
tests/golden), the number of output lines and the md5 of stdout in tests/golden/SUFFIX_MANIFEST.json -- and stdout itself where it
is at most 4 kB, so that a test without a device can compare line by line (data only; tests/test_gpu_suffix.py compares the CLI
with it, tests/test_cpu_suffix.py checks what the manifest must hold and restates the walk).  "matrix" marks the regular matrix.
    python tools/make_golden_suffix.py"""
import hashlib, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "SUFFIX_MANIFEST.json")

INDEXES = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
           "edge_dups.fmd", "longruns.fmd", "copies3000.fmd", "reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"]   # the last three hold one strand
QUERIES = [([], "mem_mutated.fa.gz"), ([], "reads_fq.fa.gz"), (["-L"], "edge_chars.txt"), ([], "mem_iupac.fa"), ([], "sw_reads.fa")]
TEXT_MAX = 4096


def cases():
    for idx in INDEXES:                                     # the regular matrix
        for qopt, q in QUERIES:
            yield qopt, [idx, q], True
    yield [], ["genomes12.fmd", "genomes12_part1.fa.gz"], False          # whole indexed records: 20 000 dependent steps each, start 0
    yield ["-L"], ["genomes12.fmd", "edge_chars.txt", "edge_dups.txt", "edge_chars.txt"], False   # seq<N> runs on over the files


man = {}
t0 = time.time()
for opts, files, matrix in cases():
    key = " ".join(opts + files)
    r = subprocess.run([ref, "suffix"] + opts + [os.path.join(GOLDEN, f) for f in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0:
        sys.exit("the reference failed on %s" % key)
    e = {"opts": opts, "files": files, "matrix": matrix, "lines": r.stdout.count(b"\n"), "md5": hashlib.md5(r.stdout).hexdigest()}
    if len(r.stdout) <= TEXT_MAX:
        e["stdout"] = r.stdout.decode("latin-1")
    man[key] = e
print("%d cases in %.1f s; %d with their text" % (len(man), time.time() - t0, sum(1 for e in man.values() if "stdout" in e)), file=sys.stderr)
json.dump(man, open(man_fn, "w"), indent=0, sort_keys=True)
open(man_fn, "a").write("\n")
