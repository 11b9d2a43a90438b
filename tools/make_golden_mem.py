#!/usr/bin/env python3
"""Golden answers of the reference's `mem` on the committed indexes and query files: runs the unmodified reference binary
(oracle/_ref/ropebwt3, built by oracle/Makefile) on every case and records the arguments, the number of output lines and the md5 of
stdout in tests/golden/MEM_MANIFEST.json (data only; tests/test_gpu_mem.py compares the CLI with it, tests/test_cpu_mem.py checks what
the manifest must hold).  "opts" are the options, "files" the index and the query files (names under tests/golden); "matrix" marks the
regular matrix; "refused" the forward-only indexes, on which the reference prints its message and nothing else.
    python tools/make_golden_mem.py"""
import hashlib, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "MEM_MANIFEST.json")

SYMMETRIC = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
             "edge_dups.fmd", "longruns.fmd", "copies3000.fmd"]
FORWARD_ONLY = ["reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"]
QUERIES = [([], "mem_mutated.fa.gz"), ([], "reads_fq.fa.gz"), (["-L"], "edge_chars.txt"), ([], "mem_iupac.fa")]


def cases():
    for idx in SYMMETRIC:                                   # the regular matrix
        for qopt, q in QUERIES:
            for l in (1, 5, 19, 31, 200):
                for c in (1, 2, 50):
                    yield ["-l%d" % l, "-c%d" % c] + qopt, [idx, q], True
    for idx in SYMMETRIC:                                   # the other outputs and options, on queries that match in the index
        big = idx.startswith("genomes12")
        q, lo = ("reads_fq.fa.gz", "-l31") if idx == "reads_fq.fmd" else ("mem_mutated.fa.gz", "-l31") if big else ("mem_iupac.fa", "-l5")
        yield ["--gap=20", lo], [idx, q], False
        yield ["--gap=50", "-l19", "-c2"], [idx, "mem_iupac.fa"], False
        yield ["--gap=300"], [idx, "mem_iupac.fa"], False  # (a query without matches is one gap)
        yield ["--cov", lo], [idx, q], False
        yield ["--cov", "-l7", "-c2"], [idx, q], False
        yield ["--cov", "--gap=20", lo], [idx, q], False   # (--gap wins)
        yield ["-K", "1k", lo], [idx, q], False            # many batches
        yield ["-K1", "-l5"], [idx, "mem_iupac.fa"], False
        yield ["-t3", lo] + (["-M"] if idx.endswith(".fmd") else []), [idx, q], False   # accepted and ignored (the reference maps FMD files only)
    yield ["-l19"], ["genomes12.fmd", "genomes12_part1.fa.gz"], False
    yield ["-l19"], ["genomes12.fmd", "mem_iupac.fa", "mem_mutated.fa.gz"], False
    yield ["-L", "-l1"], ["genomes12.fmd", "edge_chars.txt", "edge_dups.txt", "edge_chars.txt"], False   # seq<N> runs on over the files
    yield ["-L", "-l5", "-c2", "-K", "100"], ["reads_fq.fmd", "edge_chars.txt", "k4_readme.txt", "edge_chars.txt"], False
    yield ["-L", "--gap=3", "-l5"], ["edge_chars.fmd", "edge_chars.txt", "edge_dups.txt"], False
    yield ["-L", "--cov", "-l3"], ["edge_dups.fmd", "edge_chars.txt", "edge_dups.txt"], False
    yield ["-l31", "-c2"], ["reads_fq.fmd", "reads_fq.fa.gz", "mem_mutated.fa.gz"], False
    for idx in FORWARD_ONLY:
        yield ["-l19"], [idx, "mem_iupac.fa"], False


man = {}
t0 = time.time()
for opts, files, matrix in cases():
    key = " ".join(opts + files)
    if key in man:
        continue
    r = subprocess.run([ref, "mem"] + opts + [os.path.join(GOLDEN, f) for f in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    e = {"opts": opts, "files": files, "matrix": matrix, "lines": r.stdout.count(b"\n"), "md5": hashlib.md5(r.stdout).hexdigest()}
    if files[0] in FORWARD_ONLY:
        e["refused"] = [l for l in r.stderr.decode().splitlines() if l.startswith("ERROR")][0]
    elif r.returncode != 0:
        sys.exit("the reference failed on %s" % key)
    if r.stdout and e["lines"] <= 4000:      # the largest count of occurrences among the matches (cases of few lines only)
        cols = [l.split(b"\t") for l in r.stdout.splitlines()]
        if "--cov" not in opts and not any(o.startswith("--gap") for o in opts):
            e["max_size"] = max(int(c[3]) for c in cols)
    man[key] = e
print("%d cases in %.1f s; %d with output" % (len(man), time.time() - t0, sum(1 for e in man.values() if e["lines"])), file=sys.stderr)
json.dump(man, open(man_fn, "w"), indent=0, sort_keys=True)
open(man_fn, "a").write("\n")
