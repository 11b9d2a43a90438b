#!/usr/bin/env python3
"""Golden answers of the reference's `sw` with its MEM pre-filter (-j above the end length: rb3_sw aligns a query only if
rb3_fmd_smem_present finds an exact match of -j symbols, bwa-sw.c:536-539): runs the unmodified reference binary (oracle/_ref/ropebwt3,
built by oracle/Makefile) in a temporary directory, as tools/make_golden_sw.py and tools/make_golden_swlocal.py do -- the index copied
there, <index>.len.gz from the committed tests/golden/<stem>.len.gz, <index>.ssa from the committed file of that sample rate or
`ropebwt3 ssa -s S` -- and records options, files, S (null: the index as it lies, without side files), the number of lines and the md5
of stdout in tests/golden/SWSEED_MANIFEST.json (data only; tests/test_gpu_swseed.py compares the CLI with it, tests/test_cpu_swseed.py
checks what it must hold).  The options are the reference's, -j alone: this project's CLI gets `--prefilter` (and `--local` where there
is no -e, --all-e2e or -g) in front of them.  Every case is run a second time without its -j: "twin_lines" and "twin_md5" are the
unfiltered answer.  "bites" marks the cases where the filter must change the output: the tool refuses to write anything if such a case
equals its twin or is empty.  "matrix" marks the biting cases on the read fixture and the other indexes; the rest is also compared
with the live reference by the GPU test.  The stdout of the cases marked "model" (at most 300 lines, and at most 300 in the twin) goes
to tests/golden/SWSEED_STDOUT.json together with the twin's, under the twin's key (the same key without -j), where
tests/test_cpu_swseed.py holds tests/seed_model.py against the pair.
    python tools/make_golden_swseed.py"""
import hashlib, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "SWSEED_MANIFEST.json")
out_fn = os.path.join(GOLDEN, "SWSEED_STDOUT.json")

SSA = {("genomes12.fmd", 8): "genomes12.s8.ssa", ("k3_both.fmd", 0): "k3_both.s0.ssa"}   # committed, written by the reference
BITES = [["-e", "-j20"], ["-e", "-j30"], ["-e", "-j60"], ["-e", "-j100"], ["-e", "-u", "-j30"], ["-e", "-k5", "-j25"],
         ["-j20"], ["-j40"], ["-u", "-j40"], ["-k5", "-j30"], ["-g2", "-b", "-j30"]]
OTHER_IDX = [("genomes12_first6.fmd", None), ("genomes12_first6.fmr", None), ("reads_fq.fmd", None), ("k4_readme.fmd", 3)]
MODEL_MAX_LINES = 300


def cases():
    """(options, files, S, matrix, bites, stdout kept for the model)"""
    g, q = "genomes12.fmd", "sw_reads.fa"
    for o in BITES:
        yield o, [g, q], 8, True, True, o in (["-j40"], ["-u", "-j40"])
    for idx, S in OTHER_IDX:
        yield ["-e", "-j30"], [idx, q], S, True, False, False
    for o in (["-e", "-p3", "-j30"], ["-p3", "-j40"], ["-e", "-K1k", "-j30"], ["-K1k", "-j40"]):   # the budget of -p over fewer hits; batches of a kilobase
        yield o, [g, q], 8, False, True, False
    for o in (["-e", "-j30"], ["-j40"]):
        yield o, [g, q, "mem_iupac.fa"], 8, False, True, False            # seq<N> and the batches run on over the files
    for j in (20, 30):
        for u in ([], ["-u"]):
            yield ["-L", "-e"] + u + ["-j%d" % j], [g, "seed_lines.txt"], 8, False, True, True
            yield ["-L"] + u + ["-j%d" % j], [g, "seed_lines.txt"], 8, False, True, True
    for o in (["-e", "-j30"], ["-j30"]):
        yield o, [g, "mem_mutated.fa.gz"], 8, False, False, False        # queries of kilobases that all pass, through several chunks
    for o in (["-e", "-k5", "-j5"], ["-e", "-k5", "-j6"], ["-k11", "-j11"], ["-k11", "-j12"]):   # -j at the end length: no filter; one above: the filter
        yield o, [g, q], 8, False, False, False


def run(opts, files, S, tmp, made):
    idx = files[0]
    loc = os.path.join(GOLDEN, idx)
    if S is not None:
        d = os.path.join(tmp, "%s.s%d" % (idx, S))
        loc = os.path.join(d, idx)
        if d not in made:
            os.makedirs(d)
            shutil.copy(os.path.join(GOLDEN, idx), loc)
            shutil.copy(os.path.join(GOLDEN, idx.split(".")[0] + ".len.gz"), loc + ".len.gz")
            if (idx, S) in SSA:
                shutil.copy(os.path.join(GOLDEN, SSA[(idx, S)]), loc + ".ssa")
            else:
                subprocess.run([ref, "ssa", "-s%d" % S, "-o", loc + ".ssa", loc], check=True, stderr=subprocess.DEVNULL)
            made[d] = 1
    r = subprocess.run([ref, "sw"] + opts + [loc] + [os.path.join(GOLDEN, f) for f in files[1:]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    err = r.stderr.decode(errors="replace")
    if r.returncode != 0 or "BUG:" in err or any(l.startswith("ERROR") for l in err.splitlines()):
        sys.exit("the reference failed on %s: %s" % (" ".join(opts + files), err[-300:]))
    return r.stdout


def key_of(opts, files, S):
    return ("" if S is None else "-s%d " % S) + " ".join(opts + files)


def main():
    man, outs, twins = {}, {}, {}
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="swseed_")
    made = {}
    try:
        for opts, files, S, matrix, bites, keep in cases():
            key = key_of(opts, files, S)
            if key in man:
                continue
            if sum(1 for o in opts if o.startswith("-j")) != 1 or "--prefilter" in opts:
                sys.exit("a case has the reference's -j, once: %s" % key)
            bare = [o for o in opts if not o.startswith("-j")]
            tkey = key_of(bare, files, S)
            if tkey not in twins:
                twins[tkey] = run(bare, files, S, tmp, made)
            out, twin = run(opts, files, S, tmp, made), twins[tkey]
            if bites and (out == twin or not out):
                sys.exit("the filter does not bite on %s: nothing is written" % key)
            e = {"opts": opts, "files": files, "S": S, "matrix": matrix, "bites": bites, "lines": out.count(b"\n"), "md5": hashlib.md5(out).hexdigest(),
                 "twin": tkey, "twin_lines": twin.count(b"\n"), "twin_md5": hashlib.md5(twin).hexdigest()}
            if keep and 0 < e["lines"] <= MODEL_MAX_LINES and e["twin_lines"] <= MODEL_MAX_LINES:
                e["model"] = True
                outs[key], outs[tkey] = out.decode(), twin.decode()
            man[key] = e
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("%d cases in %.1f s; %d bite, %d for the model" % (len(man), time.time() - t0, sum(1 for e in man.values() if e["bites"]), sum(1 for e in man.values() if e.get("model"))),
          file=sys.stderr)
    for fn, d in ((man_fn, man), (out_fn, outs)):
        json.dump(d, open(fn, "w"), indent=0, sort_keys=True)
        open(fn, "a").write("\n")


if __name__ == "__main__":
    main()
