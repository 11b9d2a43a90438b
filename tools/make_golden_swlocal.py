#!/usr/bin/env python3
"""Golden answers of the reference's `sw` in its default, local mode: runs the unmodified reference binary (oracle/_ref/ropebwt3, built by
oracle/Makefile) in a temporary directory, as tools/make_golden_sw.py does for the end-to-end mode -- the index copied there, <index>.len.gz
from the committed tests/golden/<stem>.len.gz, <index>.ssa from `ropebwt3 ssa -s S` -- and records options, files, S (null: the index as
it lies, without side files), the number of lines and the md5 of stdout in tests/golden/SWLOCAL_MANIFEST.json (data only;
tests/test_gpu_swlocal.py compares `sw --local` with it, tests/test_cpu_swlocal.py checks what it must hold).  The options are the
reference's: this project's CLI gets `--local` in front of them.  "matrix" marks the regular matrix, "refused" the forward-only indexes,
"nolen" a case whose .len.gz is withheld.  The stdout itself of the cases marked "model" (at most 300 lines, an index whose plain BWT is
committed) goes to tests/golden/SWLOCAL_STDOUT.json, where tests/test_cpu_swlocal.py holds tests/swlocal_model.py against it.  The tool
stops if the reference exits non-zero or prints a line with BUG: (its backtrack's complaint about an F step without a column).
    python tools/make_golden_swlocal.py"""
import hashlib, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "SWLOCAL_MANIFEST.json")
out_fn = os.path.join(GOLDEN, "SWLOCAL_STDOUT.json")

SYMMETRIC = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
             "edge_dups.fmd", "longruns.fmd", "copies3000.fmd"]
FORWARD_ONLY = ["reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"]
SIDE = {"genomes12.fmd": 8, "k3_both.fmd": 0, "k4_readme.fmd": 3, "edge_dups.fmd": 3, "longruns.fmd": 8, "copies3000.fmd": 8}   # the sample rate of the matrix cases
QUERIES = [([], "sw_reads.fa"), ([], "mem_iupac.fa"), (["-L"], "edge_chars.txt")]
OPTS = [[], ["-k5"], ["-N5"], ["-m10", "-k3"]]
MODEL_IDX = ["genomes12.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd", "edge_dups.fmd"]   # their plain BWT is committed
MODEL_MAX_LINES = 300
MODEL = "model"


def cases():
    """(options, files, S, matrix, nolen, stdout kept for the model)"""
    for idx in SYMMETRIC:
        for qopt, q in QUERIES:
            for o in OPTS:
                yield o + qopt, [idx, q], SIDE.get(idx), True, False, True
    g, q = "genomes12.fmd", "sw_reads.fa"
    for S in (0, 3, 8):
        for p in (1, 3, 50):
            yield ["-p%d" % p], [g, q], S, False, False, False
    yield ["--no-ssa"], [g, q], 8, False, False, False
    yield [], [g, q], 8, False, True, False                    # .ssa without .len.gz: string numbers in the columns
    yield ["-p4"], [g, "mem_iupac.fa"], 8, False, True, False  # -p needs both files
    for o in (["-u"], ["--seq"], ["-N1"], ["-N200"], ["-A2", "-B4", "-O4", "-E1"], ["-K1k"], ["-t3", "-C", "1k", "-M", "-b", "-y3"], ["-j5"]):
        yield o, [g, q], 8, False, False, o in (["-N1"], ["-A2", "-B4", "-O4", "-E1"])
    yield ["-u", "--seq", "-p3", "-m10", "-k3"], [g, "mem_iupac.fa"], 8, False, False, True   # N of the query counted as A: *ng, *nc
    yield ["-N200", "-m10", "-k3", "-p2"], [g, "mem_iupac.fa"], 8, False, False, True   # rows and table in global memory, on a handful of queries
    yield [], [g, q, "mem_iupac.fa"], 8, False, False, False   # seq<N> and the batches run on over the files
    yield ["-L", "-u", "-m3", "-k2"], [g, "edge_chars.txt", "edge_dups.txt", "edge_chars.txt"], 8, False, False, True
    for idx in ("copies3000.fmd", "genomes12.fmd", "longruns.fmd"):
        yield ["-L", "-m5", "-k2"], [idx, "sw_runs.txt"], 8, False, False, True    # repeats inside the query: qh:i above 1
    yield ["-L", "-m5", "-k2", "-p5"], ["longruns.fmd", "sw_runs.txt"], 3, False, False, False
    yield [], ["reads_fq.fmd", "reads_fq.fa.gz"], None, False, False, False
    yield ["-m10", "-k3"], [g, "reads_fq.fa.gz"], 8, False, False, False
    yield [], [g, "mem_mutated.fa.gz"], 8, False, False, False   # queries of kilobases: thousands of nodes
    for idx in FORWARD_ONLY:
        yield [], [idx, "mem_iupac.fa"], None, False, False, False


def paf_counts(text):
    c = dict(I=0, D=0, X=0, minus=0, ap=0, qh=0, unmapped=0, rh_max=0)
    for l in text.splitlines():
        f = l.split("\t")
        if f[2] == "*":
            c["unmapped"] += 1
            continue
        cg = [x for x in f[12:] if x.startswith("cg:Z:")][0]
        for k in "IDX":
            c[k] += k in cg
        c["minus"] += f[4] == "-"
        c["ap"] += any(x.startswith("ap:Z:") for x in f[12:])
        c["qh"] += any(x.startswith("qh:i:") and int(x[5:]) > 1 for x in f[12:])
        c["rh_max"] = max([c["rh_max"]] + [int(x[5:]) for x in f[12:] if x.startswith("rh:i:")])
    return c


def main():
    man, outs = {}, {}
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="swlocal_")
    made = {}
    try:
        for opts, files, S, matrix, nolen, keep in cases():
            key = ("" if S is None else "-s%d " % S) + ("nolen " if nolen else "") + " ".join(opts + files)
            if key in man:
                continue
            idx = files[0]
            loc = os.path.join(GOLDEN, idx)
            if S is not None:
                d = os.path.join(tmp, "%s.s%d%s" % (idx, S, ".nolen" if nolen else ""))
                loc = os.path.join(d, idx)
                if d not in made:
                    os.makedirs(d)
                    shutil.copy(os.path.join(GOLDEN, idx), loc)
                    if not nolen:
                        shutil.copy(os.path.join(GOLDEN, idx.split(".")[0] + ".len.gz"), loc + ".len.gz")
                    subprocess.run([ref, "ssa", "-s%d" % S, "-o", loc + ".ssa", loc], check=True, stderr=subprocess.DEVNULL)
                    made[d] = 1
            r = subprocess.run([ref, "sw"] + opts + [loc] + [os.path.join(GOLDEN, f) for f in files[1:]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            e = {"opts": opts, "files": files, "S": S, "matrix": matrix, "nolen": nolen, "lines": r.stdout.count(b"\n"), "md5": hashlib.md5(r.stdout).hexdigest()}
            err = r.stderr.decode(errors="replace")
            if "BUG:" in err:
                sys.exit("the reference printed BUG: on %s" % key)
            errs = [l for l in err.splitlines() if l.startswith("ERROR")]
            if errs:
                e["refused"] = errs[0]
                if r.stdout:
                    sys.exit("the reference refused %s and wrote something" % key)
            elif r.returncode != 0:
                sys.exit("the reference failed on %s: %s" % (key, err[-300:]))
            if not errs:
                e["counts"] = paf_counts(r.stdout.decode())
            if keep and idx in MODEL_IDX and 0 < e["lines"] <= MODEL_MAX_LINES:
                e[MODEL] = True
                outs[key] = r.stdout.decode()
            man[key] = e
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("%d cases in %.1f s; %d with output, %d for the model" % (len(man), time.time() - t0, sum(1 for e in man.values() if e["lines"]), len(outs)), file=sys.stderr)
    for fn, d in ((man_fn, man), (out_fn, outs)):
        json.dump(d, open(fn, "w"), indent=0, sort_keys=True)
        open(fn, "a").write("\n")


if __name__ == "__main__":
    main()
