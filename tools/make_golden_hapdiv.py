#!/usr/bin/env python3
"""Golden answers of the reference's `hapdiv` on the committed indexes and query files: runs the unmodified reference binary
(oracle/_ref/ropebwt3, built by oracle/Makefile) on every case and records the options, the files, the number of output lines and the
md5 of stdout in tests/golden/HAPDIV_MANIFEST.json (data only; tests/test_gpu_hapdiv.py compares the CLI with it, tests/test_cpu_hapdiv.py
checks what the manifest must hold).  "matrix" marks the regular matrix; "refused" the forward-only indexes, on which the reference
prints its message and nothing else.  The stdout itself of the cases marked "model" (few lines, an index whose plain BWT is committed)
goes to tests/golden/HAPDIV_STDOUT.json, where tests/test_cpu_hapdiv.py holds tests/sw_model.py against it window by window.
    python tools/make_golden_hapdiv.py"""
import hashlib, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "HAPDIV_MANIFEST.json")
out_fn = os.path.join(GOLDEN, "HAPDIV_STDOUT.json")

SYMMETRIC = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
             "edge_dups.fmd", "longruns.fmd", "copies3000.fmd"]
FORWARD_ONLY = ["reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"]
QUERIES = [([], "mem_mutated.fa.gz"), ([], "mem_iupac.fa"), ([], "reads_fq.fa.gz"), (["-L"], "edge_chars.txt")]
OPTS = [[], ["-a31", "-w7"], ["-a51", "-w10", "-N5"], ["-a31", "-w1", "-N3"], ["-N1"]]
MODEL_IDX = ["genomes12.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd", "edge_dups.fmd"]   # their plain BWT is committed
MODEL_MAX_LINES = 300


def cases():
    for idx in SYMMETRIC:                                   # the regular matrix
        for qopt, q in QUERIES:
            for o in OPTS:
                yield o + qopt, [idx, q], True, idx in MODEL_IDX and q in ("mem_iupac.fa", "edge_chars.txt")
    g, q = "genomes12.fmd", "mem_mutated.fa.gz"
    yield ["-N200"], [g, q], False, False
    yield ["-a1", "-w1"], [g, q], False, False
    yield ["-a1", "-w1", "-m1"], [g, "mem_iupac.fa"], False, True
    yield ["-m1", "-a20"], [g, q], False, False
    yield ["-m1", "-a20"], [g, "mem_iupac.fa"], False, True
    yield ["-y2"], [g, q], False, False
    yield ["-y0"], [g, q], False, False
    yield ["-y2", "-a40", "-m20"], [g, "mem_iupac.fa"], False, True
    yield ["-A2", "-B4", "-O4", "-E1"], [g, q], False, False
    yield ["-A2", "-B4", "-O4", "-E1", "-a40", "-m20"], [g, "mem_iupac.fa"], False, True
    yield ["-a5000"], [g, q], False, False
    yield ["-K1k"], [g, q], False, False
    yield ["-t3", "-C", "1k", "-M"], [g, q], False, False              # accepted and ignored
    yield ["-e", "-k5", "-b", "-u", "-j30", "-l40", "--seq"], [g, q], False, False   # hapdiv is end to end with end_len 1 whatever these say
    yield ["-a31", "-w7"], [g, "mem_iupac.fa", q], False, False
    yield ["-L", "-a5", "-w1", "-m1"], [g, "edge_chars.txt", "edge_dups.txt", "edge_chars.txt"], False, False   # seq<N> runs on over the files
    yield ["-L", "-a5", "-w1", "-m1", "-K", "100"], ["reads_fq.fmd", "edge_chars.txt", "k4_readme.txt", "edge_chars.txt"], False, False
    yield ["-a31", "-w7", "-N4"], ["copies3000.fmd", q], False, False  # intervals of a million rows
    yield ["-a31", "-w7", "-N4"], ["longruns.fmd", q], False, False
    for idx in FORWARD_ONLY:
        yield [], [idx, "mem_iupac.fa"], False, False


man, outs = {}, {}
t0 = time.time()
for opts, files, matrix, model in cases():
    key = " ".join(opts + files)
    if key in man:
        continue
    r = subprocess.run([ref, "hapdiv"] + opts + [os.path.join(GOLDEN, f) for f in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    e = {"opts": opts, "files": files, "matrix": matrix, "lines": r.stdout.count(b"\n"), "md5": hashlib.md5(r.stdout).hexdigest()}
    if files[0] in FORWARD_ONLY:
        e["refused"] = [l for l in r.stderr.decode().splitlines() if l.startswith("ERROR")][0]
    elif r.returncode != 0:
        sys.exit("the reference failed on %s" % key)
    if model and 0 < e["lines"] <= MODEL_MAX_LINES:
        e["model"] = True
        outs[key] = r.stdout.decode()
    man[key] = e
print("%d cases in %.1f s; %d with output, %d for the model" % (len(man), time.time() - t0, sum(1 for e in man.values() if e["lines"]), len(outs)), file=sys.stderr)
for fn, d in ((man_fn, man), (out_fn, outs)):
    json.dump(d, open(fn, "w"), indent=0, sort_keys=True)
    open(fn, "a").write("\n")
