#!/usr/bin/env python3
"""Golden answers for `remove`: what is left of a committed index after sequences are taken out must be, byte for byte, the index the reference builds
from the sequences that stay.  For every case the inputs of the index (tests/golden/MANIFEST.json: files and flags) are read, the records named are
left out, the unmodified reference binary (oracle/_ref/ropebwt3, built by oracle/Makefile) runs `build -d <flags>` on the rest, and the md5 and byte count
of that FMD go to tests/golden/REMOVE_MANIFEST.json -- data only: case name, index, rows (inclusive ranges of string numbers, i.e. rows below acc[1]),
md5 and byte count.  tests/test_gpu_remove.py compares the CLI with it, on both marking paths.
    python tools/make_golden_remove.py"""
import gzip, hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
MAN = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
INDEXES = ["edge_chars", "edge_dups", "k2_fwd", "k3_both", "k4_readme", "copies3000", "longruns", "reads_fwd", "reads_rev", "reads_fq", "genomes12"]


def records(fn, is_line):
    """the sequences of an input file in order: lines (-L), FASTA or FASTQ"""
    data = (gzip.open(fn).read() if fn.endswith(".gz") else open(fn, "rb").read()).decode("latin-1")
    lines = data.split("\n")
    if is_line:
        return [x.strip() for x in lines if x.strip()]
    out, i = [], 0
    while i < len(lines):
        if lines[i].startswith(">"):
            j = i + 1
            while j < len(lines) and not lines[j].startswith(">"):
                j += 1
            out.append("".join(x.strip() for x in lines[i + 1:j]))
            i = j
        elif lines[i].startswith("@"):
            out.append(lines[i + 1].strip())
            i += 4
        else:
            i += 1
    return out


def ranges(xs):
    out = []
    for x in sorted(xs):
        if out and out[-1][1] == x - 1:
            out[-1][1] = x
        else:
            out.append([x, x])
    return out


def subsets(n):
    """(name, sequences taken out) of an index of n sequences"""
    yield "first", [0]
    yield "last", [n - 1]
    yield "middle", [n // 2]
    yield "every_second", list(range(0, n, 2)) if n > 2 else [0]
    yield "all_but_one", [i for i in range(n) if i != n // 3]


man = {}
tmp = tempfile.mkdtemp(prefix="rb3_remove_golden_")
for name in INDEXES:
    e = MAN[name]
    flags = [f for f in e["flags"] if f in ("-L", "-R", "-F")]
    both = "-R" not in flags and "-F" not in flags
    recs = []
    for inp in e["inputs"]:
        recs += records(os.path.join(GOLDEN, inp), "-L" in flags)
    n = len(recs)
    assert sum(len(s) + 1 for s in recs) * (2 if both else 1) == e["n_symbols"], name    # the records read here are the strings of the index
    todo = list(subsets(n))
    if name == "genomes12":    # the halves of the resume fixture: what stays is genomes12_rest6.fa.gz / genomes12_first6.fa.gz
        todo = [("first6", list(range(0, 6))), ("rest6", list(range(6, 12))), ("middle", [5])]
    if n == 1 and both:        # one sequence: a strand of it goes, and what stays is the reference's build of the other strand alone (-R / -F)
        for case, row, flag in (("drop_reverse", 1, "-R"), ("drop_forward", 0, "-F")):
            fn = os.path.join(tmp, "%s_%s.fa" % (name, case))
            open(fn, "w").write(">0\n%s\n" % recs[0])
            r = subprocess.run([ref, "build", "-t4", "-d", flag, fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            man["%s/%s" % (name, case)] = {"case": case, "index": e["fmd"], "rows": [[row, row]], "md5": hashlib.md5(r.stdout).hexdigest(), "bytes": len(r.stdout)}
            os.remove(fn)
        continue
    for case, out_seqs in todo:
        gone = set(out_seqs)
        assert gone and len(gone) < n and max(gone) < n, (name, case, n)
        fn = os.path.join(tmp, "%s_%s.fa" % (name, case))
        with open(fn, "w") as fp:
            for i, s in enumerate(recs):
                if i not in gone:
                    fp.write(">%d\n%s\n" % (i, s))
        r = subprocess.run([ref, "build", "-t4", "-d"] + [f for f in flags if f != "-L"] + [fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            sys.exit("the reference failed on %s/%s: %s" % (name, case, r.stderr.decode()[-500:]))
        rows = ranges([2 * i + k for i in gone for k in (0, 1)] if both else list(gone))
        man["%s/%s" % (name, case)] = {"case": case, "index": e["fmd"], "rows": rows, "md5": hashlib.md5(r.stdout).hexdigest(), "bytes": len(r.stdout)}
        os.remove(fn)
os.rmdir(tmp)
first6 = open(os.path.join(GOLDEN, "genomes12_first6.fmd"), "rb").read()
assert man["genomes12/rest6"]["md5"] == hashlib.md5(first6).hexdigest(), "genomes12 without its last six is not the committed genomes12_first6.fmd"
with open(os.path.join(GOLDEN, "REMOVE_MANIFEST.json"), "w") as fp:    # one case per line
    fp.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(man[k], sort_keys=True, separators=(",", ":"))) for k in sorted(man)) + "\n}\n")
print("%d cases -> tests/golden/REMOVE_MANIFEST.json" % len(man))
