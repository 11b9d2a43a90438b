#!/usr/bin/env python3
"""Golden answers of the reference's `mem -p` (positions of the matches): runs the unmodified reference binary (oracle/_ref/ropebwt3, built by
oracle/Makefile) in a temporary directory -- the index copied there, <index>.len.gz written from the committed source of the index,
`ropebwt3 ssa -s S` for <index>.ssa, then `mem -p` -- and records options, files, S, the number of lines, the md5 of stdout and the
largest count of occurrences in tests/golden/MEMPOS_MANIFEST.json (data only; tests/test_gpu_mempos.py compares the CLI with it).  Cases
of few lines also keep their lines ("out"): tests/test_cpu_mempos.py pins tests/pos_model.py on them.  The name lists are committed as
tests/golden/<stem>.len.gz -- never as <index>.len.gz, which would change what `mem -p <golden index>` does in the existing tests.
    python tools/make_golden_mempos.py"""
import gzip, hashlib, io, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ref = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
man_fn = os.path.join(GOLDEN, "MEMPOS_MANIFEST.json")

# index -> (the text it was built from, the committed .ssa files written by the reference: S -> name)
SOURCES = {"genomes12.fmd": ("genomes12.fa.gz", {8: "genomes12.s8.ssa"}), "copies3000.fmd": ("copies3000.txt.gz", {}), "edge_dups.fmd": ("edge_dups.txt", {}),
           "longruns.fmd": ("longruns.txt.gz", {}), "k4_readme.fmd": ("k4_readme.txt", {}), "k3_both.fmd": ("k3_both.txt", {0: "k3_both.s0.ssa"})}
SHIFTS = (0, 3, 8)


def names_lengths(fn):
    """the records of a FASTA / FASTQ / one-per-line file as the reference's reader names them (the name ends at the first blank)"""
    raw = open(fn, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    lines = raw.split(b"\n")
    out = []
    stem = os.path.basename(fn).split(".")[0]
    if raw[:1] == b">":
        for l in lines:
            if l[:1] == b">":
                out.append([l[1:].split()[0].decode(), 0])
            elif out:
                out[-1][1] += len(l.strip())
    elif raw[:1] == b"@":
        for i in range(0, len(lines) - 3, 4):
            out.append([lines[i][1:].split()[0].decode(), len(lines[i + 1].strip())])
    else:
        out = [["%s_%d" % (stem, i), len(l.strip())] for i, l in enumerate(lines) if l.strip()]
    return out


def len_gz(idx):
    src = SOURCES[idx][0]
    nl = names_lengths(os.path.join(GOLDEN, src))
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0, filename="") as f:
        f.write("".join("%s\t%d\n" % (n, l) for n, l in nl).encode())
    fn = os.path.join(GOLDEN, idx.split(".")[0] + ".len.gz")
    open(fn, "wb").write(buf.getvalue())
    return fn


def cases():
    g = "genomes12.fmd"
    for S in SHIFTS:
        for p in (1, 5, 1000):
            yield ["-l19", "-p%d" % p], [g, "mem_mutated.fa.gz"], S
        yield ["-l5", "-c2", "-p20"], [g, "mem_mutated.fa.gz"], S           # P below the size: the traversal chooses
        yield ["-l31", "-p10"], [g, "mem_iupac.fa"], S                      # both strands in the columns
        yield ["-l1", "-p3"], [g, "mem_iupac.fa"], S                        # matches of size 0: no extra column
        yield ["-K", "1k", "-l19", "-p5"], [g, "mem_mutated.fa.gz"], S
        yield ["-l19", "-p4"], [g, "mem_iupac.fa", "mem_mutated.fa.gz"], S
        yield ["-L", "-l1", "-p6"], [g, "edge_chars.txt", "edge_dups.txt"], S
        yield ["--gap=20", "-l31", "-p5"], [g, "mem_mutated.fa.gz"], S      # --gap switches -p off
        yield ["--cov", "-l31", "-p5"], [g, "mem_mutated.fa.gz"], S         # --cov needs the files and prints no positions
        for idx in ("copies3000.fmd", "edge_dups.fmd", "longruns.fmd", "k4_readme.fmd", "k3_both.fmd"):   # identical strings: large intervals, ties in the heap
            yield ["-l5", "-p3"], [idx, "mem_iupac.fa"], S
            yield ["-l3", "-c2", "-p50"], [idx, "mem_iupac.fa"], S
            yield ["-L", "-l1", "-p100"], [idx, "edge_dups.txt", "k4_readme.txt"], S
            yield ["-L", "-l2", "-p7"], [idx, os.path.basename(SOURCES[idx][0])] if not SOURCES[idx][0].endswith(".gz") else [idx, "k3_both.txt"], S
    for S in (3, 8):
        yield ["-l5", "-c2", "-p20"], [g, "reads_fq.fa.gz"], S              # volume: several output slices
        yield ["-l5", "-c2", "-p2000"], ["copies3000.fmd", "mem_mutated.fa.gz"], S


man = {}
t0 = time.time()
tmp = tempfile.mkdtemp(prefix="mempos_")
made = {}
try:
    for opts, files, S in cases():
        key = "-s%d " % S + " ".join(opts + files)
        if key in man:
            continue
        idx = files[0]
        d = os.path.join(tmp, "%s.s%d" % (idx, S))
        loc = os.path.join(d, idx)
        if (idx, S) not in made:
            os.makedirs(d)
            shutil.copy(os.path.join(GOLDEN, idx), loc)
            shutil.copy(len_gz(idx), loc + ".len.gz")
            subprocess.run([ref, "ssa", "-s%d" % S, "-o", loc + ".ssa", loc], check=True, stderr=subprocess.DEVNULL)
            gold = SOURCES[idx][1].get(S)
            if gold and open(os.path.join(GOLDEN, gold), "rb").read() != open(loc + ".ssa", "rb").read():
                sys.exit("%s is not what the reference writes today" % gold)
            made[(idx, S)] = 1
        r = subprocess.run([ref, "mem"] + opts + [loc] + [os.path.join(GOLDEN, f) for f in files[1:]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        if r.returncode != 0 or b"ERROR" in r.stderr:
            sys.exit("the reference failed on %s: %s" % (key, r.stderr.decode()[-300:]))
        e = {"opts": opts, "files": files, "S": S, "ssa": SOURCES[idx][1].get(S), "len": idx.split(".")[0] + ".len.gz", "lines": r.stdout.count(b"\n"), "md5": hashlib.md5(r.stdout).hexdigest()}
        plain = "--cov" in opts or any(o.startswith("--gap") for o in opts)
        if r.stdout and not plain and e["lines"] <= 20000:
            e["max_size"] = max(int(l.split(b"\t")[3]) for l in r.stdout.splitlines())
        if not plain and 0 < e["lines"] <= 12 and len(r.stdout) < 6000:
            e["out"] = r.stdout.decode()
        man[key] = e
finally:
    shutil.rmtree(tmp, ignore_errors=True)
print("%d cases in %.1f s; %d with output" % (len(man), time.time() - t0, sum(1 for e in man.values() if e["lines"])), file=sys.stderr)
json.dump(man, open(man_fn, "w"), indent=0, sort_keys=True)
open(man_fn, "a").write("\n")
