#!/usr/bin/env python3
"""Golden answers of the reference's `sw` in end-to-end mode (-e, --all-e2e, -g): runs the unmodified reference binary (oracle/_ref/ropebwt3,
built by oracle/Makefile) in a temporary directory -- the index copied there, <index>.len.gz from the committed tests/golden/<stem>.len.gz,
<index>.ssa from the committed file of that sample rate or `ropebwt3 ssa -s S` -- and records options, files, S (null: the index as it
lies, without side files), the number of lines and the md5 of stdout in tests/golden/SW_MANIFEST.json (data only; tests/test_gpu_sw.py
compares the CLI with it, tests/test_cpu_sw.py checks what it must hold).  "matrix" marks the regular matrix, "refused" the forward-only
indexes, "nolen" a case whose .len.gz is withheld.  The stdout itself of the cases marked "model" (at most 300 lines, an index whose
plain BWT is committed) goes to tests/golden/SW_STDOUT.json, where tests/test_cpu_sw.py holds tests/swaln_model.py against it.
    python tools/make_golden_sw.py"""
import hashlib, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "SW_MANIFEST.json")
out_fn = os.path.join(GOLDEN, "SW_STDOUT.json")

SYMMETRIC = ["genomes12.fmd", "genomes12_first6.fmd", "genomes12_first6.fmr", "reads_fq.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd",
             "edge_dups.fmd", "longruns.fmd", "copies3000.fmd"]
FORWARD_ONLY = ["reads_fwd.fmd", "reads_rev.fmd", "k2_fwd.fmd"]
# index -> (the sample rate of its matrix cases, the committed .ssa files written by the reference: S -> name); its name list is <stem>.len.gz
SIDE = {"genomes12.fmd": (8, {8: "genomes12.s8.ssa"}), "k3_both.fmd": (0, {0: "k3_both.s0.ssa"}), "k4_readme.fmd": (3, {}), "edge_dups.fmd": (3, {}),
        "longruns.fmd": (8, {}), "copies3000.fmd": (8, {})}
QUERIES = [([], "sw_reads.fa"), ([], "mem_iupac.fa"), (["-L"], "edge_chars.txt")]
OPTS = [["-e"], ["-e", "-N5"], ["--all-e2e", "-b"]]
MODEL_IDX = ["genomes12.fmd", "k3_both.fmd", "k4_readme.fmd", "edge_chars.fmd", "edge_dups.fmd"]   # their plain BWT is committed
MODEL_MAX_LINES = 300


def cases():
    """(options, files, S, matrix, nolen)"""
    for idx in SYMMETRIC:
        for qopt, q in QUERIES:
            for o in OPTS:
                yield o + qopt, [idx, q], SIDE[idx][0] if idx in SIDE else None, True, False
    g, q = "genomes12.fmd", "sw_reads.fa"
    for S in (0, 3, 8):
        for p in (1, 3, 50):                                  # budgets used up in the middle of a query: later hits fall back to one position
            yield ["-e", "-p%d" % p], [g, q], S, False, False
        yield ["-e", "-p3"], [g, "mem_iupac.fa"], S, False, False
    yield ["-e", "--no-ssa"], [g, q], 8, False, False
    yield ["-e", "--no-ssa"], [g, "mem_iupac.fa"], 8, False, False
    yield ["-e"], [g, q], 8, False, True                      # .ssa without .len.gz: string numbers in the columns
    yield ["-e", "-p4"], [g, "mem_iupac.fa"], 8, False, True  # -p needs both files
    yield ["-e"], [g, "mem_iupac.fa"], 8, False, True
    for o in (["-e", "-k11"], ["-k5", "-e"], ["-e", "-k5"], ["-e", "-u"], ["-e", "--seq"], ["-e", "-m10", "-y4"], ["-e", "-y0"], ["-e", "-N1"], ["-e", "-N200"],
              ["-e", "-A2", "-B4", "-O4", "-E1"], ["--all-e2e", "-g3"], ["-g1", "-b"], ["-e", "-K1k"], ["-e", "-b"], ["-e", "-t3", "-C", "1k", "-M"],
              ["-e", "-u", "--seq", "-p2"]):
        yield o, [g, q], 8, False, False
    for o in (["-e", "-k11"], ["-e", "-k5"], ["-e", "-u", "--seq", "-m10"], ["-g2", "-b"], ["-e", "-A2", "-B4", "-O4", "-E1", "-m20"], ["-e", "-N1"], ["-e", "-y0", "-m20"]):
        yield o, [g, "mem_iupac.fa"], 8, False, False
    yield ["-e"], [g, q, "mem_iupac.fa"], 8, False, False     # seq<N> and the batches run on over the files
    yield ["-e", "-L", "-u", "-m3"], [g, "edge_chars.txt", "edge_dups.txt", "edge_chars.txt"], 8, False, False
    yield ["-e"], [g, "mem_mutated.fa.gz"], 8, False, False   # queries of kilobases, few hits
    for idx in ("copies3000.fmd", "longruns.fmd"):
        for S in (3, 8):                                      # intervals of a million rows
            yield ["-e", "-L", "-p5"], [idx, "sw_runs.txt"], S, False, False
        yield ["-e", "-L", "-p2000", "-N3"], [idx, "sw_runs.txt"], 8, False, False
    for idx in FORWARD_ONLY:
        yield ["-e"], [idx, "mem_iupac.fa"], None, False, False


def paf_counts(text, query_fn):
    """what tests/test_cpu_sw.py asks of the read fixture: lines with an insertion, a deletion, a mismatch in cg, on strand -, with an ap tag;
    queries without a hit and with five or more"""
    names = [l[1:].split()[0] for l in open(query_fn) if l.startswith(">")]
    per = dict.fromkeys(names, 0)
    c = dict(I=0, D=0, X=0, minus=0, ap=0)
    for l in text.splitlines():
        f = l.split("\t")
        if f[2] == "*":
            continue
        per[f[0]] += 1
        cg = [x for x in f[12:] if x.startswith("cg:Z:")][0]
        for k in "IDX":
            c[k] += k in cg
        c["minus"] += f[4] == "-"
        c["ap"] += any(x.startswith("ap:Z:") for x in f[12:])
    c["no_hit"] = sum(1 for n in per.values() if n == 0)
    c["five_plus"] = sum(1 for n in per.values() if n >= 5)
    return c


def main():
    man, outs = {}, {}
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="sw_")
    made = {}
    try:
        for opts, files, S, matrix, nolen in cases():
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
                    gold = SIDE[idx][1].get(S)
                    subprocess.run([ref, "ssa", "-s%d" % S, "-o", loc + ".ssa", loc], check=True, stderr=subprocess.DEVNULL)
                    if gold and open(os.path.join(GOLDEN, gold), "rb").read() != open(loc + ".ssa", "rb").read():
                        sys.exit("%s is not what the reference writes today" % gold)
                    made[d] = 1
            r = subprocess.run([ref, "sw"] + opts + [loc] + [os.path.join(GOLDEN, f) for f in files[1:]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            e = {"opts": opts, "files": files, "S": S, "matrix": matrix, "nolen": nolen, "lines": r.stdout.count(b"\n"), "md5": hashlib.md5(r.stdout).hexdigest()}
            errs = [l for l in r.stderr.decode().splitlines() if l.startswith("ERROR")]
            if errs:
                e["refused"] = errs[0]
                if r.stdout:
                    sys.exit("the reference refused %s and wrote something" % key)
            elif r.returncode != 0:
                sys.exit("the reference failed on %s: %s" % (key, r.stderr.decode()[-300:]))
            if files[1:] == ["sw_reads.fa"] and not errs and "--all-e2e" not in opts and not any(o.startswith("-g") for o in opts):
                e["counts"] = paf_counts(r.stdout.decode(), os.path.join(GOLDEN, files[1]))
            if idx in MODEL_IDX and 0 < e["lines"] <= MODEL_MAX_LINES:
                e["model"] = True
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
