#!/usr/bin/env python3
"""Golden answers of the reference's `hapdiv`, `sw -e` and `sw` (local) on the inputs of tests/dp_cases.py, which make the candidate table of
the dynamic program grow: writes the genome and the query sets as gzipped FASTA fixtures (tests/golden/dptable_*.fa.gz, data made by
tests/dp_cases.py from its seeds), lets the unmodified reference binary (oracle/_ref/ropebwt3, built by oracle/Makefile) index the genome
with `build -d` in a temporary directory and runs every case at every recorded n_best.  Options, file, number of lines, md5 and the
stdout itself go to tests/golden/DPTABLE_MANIFEST.json (data only): tests/test_cpu_dptable.py holds the three Python models against it,
tests/test_gpu_dptable.py the command line.  Stops if the reference fails, prints `BUG:` or answers nothing.
    python tools/make_golden_dptable.py"""
import gzip, hashlib, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dp_cases as dp

GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "DPTABLE_MANIFEST.json")


def write_fasta(fn, names, seqs):
    text = "".join(">%s\n%s\n" % (n, "".join("$ACGTN"[int(c)] for c in s)) for n, s in zip(names, seqs))
    with open(fn, "wb") as f:                       # (no name, no time in the header: the same bytes every time)
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as z:
            z.write(text.encode())


def main():
    write_fasta(os.path.join(GOLDEN, dp.GENOME_FILE), [dp.GENOME_NAME], [dp.genome()])
    for fn, make in dp.FILES.items():
        write_fasta(os.path.join(GOLDEN, fn), dp.query_names(fn), make())
    man = {}
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="dptable_")
    try:
        idx = os.path.join(tmp, "dptable_genome.fmd")
        with open(idx, "wb") as f:
            subprocess.run([ref, "build", "-d", "-t4", os.path.join(GOLDEN, dp.GENOME_FILE)], stdout=f, stderr=subprocess.DEVNULL, check=True)
        for case in dp.CASES:
            cmd = "hapdiv" if case.kernel == "hapdiv" else "sw"
            for N in case.n_list:
                if case.n_list == dp.N_LIST and N not in dp.N_RECORDED:
                    continue
                opts = case.args + ["-N%d" % N]
                key = " ".join([cmd] + opts + [case.file])
                r = subprocess.run([ref, cmd] + opts + [idx, os.path.join(GOLDEN, case.file)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
                if r.returncode != 0 or b"BUG:" in r.stderr or not r.stdout:
                    sys.exit("the reference failed on %s: %s" % (key, r.stderr.decode()[-300:]))
                man[key] = {"case": case.name, "cmd": cmd, "opts": opts, "n_best": N, "file": case.file, "lines": r.stdout.count(b"\n"),
                            "md5": hashlib.md5(r.stdout).hexdigest(), "stdout": r.stdout.decode()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("%d cases in %.1f s" % (len(man), time.time() - t0), file=sys.stderr)
    json.dump(man, open(man_fn, "w"), indent=0, sort_keys=True)
    open(man_fn, "a").write("\n")


if __name__ == "__main__":
    main()
