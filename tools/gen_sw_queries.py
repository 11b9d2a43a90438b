#!/usr/bin/env python3
"""The reads of the `sw` goldens, tests/golden/sw_reads.fa: reads of 40-130 bp cut from tests/golden/genomes12.fa.gz with a fixed seed,
half of them reverse-complemented, with 0-4 edits each (substitutions, insertions and deletions of 1-3 bp, kept 12 bp away from both
ends), every tenth read with one N, twelve reads that are too short or too damaged to align, and one random read.  And
tests/golden/sw_runs.txt, one query per line for the indexes of identical strings and long runs (copies3000, longruns), whose hits
are intervals of thousands to a million rows: pieces of their own strings, exact and with one substitution.
    python tools/gen_sw_queries.py"""
import gzip, os, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_READS, SEED, MARGIN = 240, 20260117, 12
COMP = str.maketrans("ACGTacgt", "TGCAtgca")

rng = random.Random(SEED)
genomes, name = [], None
for line in gzip.open(os.path.join(GOLDEN, "genomes12.fa.gz"), "rt"):
    if line.startswith(">"):
        genomes.append([line[1:].split()[0], []])
    else:
        genomes[-1][1].append(line.strip())
genomes = [(n, "".join(s).upper()) for n, s in genomes]


def edit(s, kind):
    at = rng.randrange(MARGIN, len(s) - MARGIN)
    if kind == "X":
        return s[:at] + rng.choice([c for c in "ACGT" if c != s[at]]) + s[at + 1:]
    n = rng.randint(1, 3)
    if kind == "I":
        return s[:at] + "".join(rng.choice("ACGT") for _ in range(n)) + s[at:]
    return s[:at] + s[min(at + n, len(s) - MARGIN):]


out = []
for i in range(N_READS):
    g_name, g = genomes[rng.randrange(len(genomes))]
    length = rng.randint(40, 130)
    st = rng.randrange(0, len(g) - length)
    s = g[st:st + length]
    strand = "+"
    if i % 2:
        s, strand = s.translate(COMP)[::-1], "-"
    if i % 20 == 7:                        # hopeless: a dozen edits, or too short for the default score
        kinds = "XXXXIDXXXXID" if i % 40 == 7 else ""
        if not kinds:
            s = s[:rng.randint(20, 28)]
    else:
        kinds = [rng.choice("XID") for _ in range(rng.choice((0, 1, 1, 2, 2, 3, 4)))]
    for kind in kinds:
        if len(s) > 2 * MARGIN + 4:
            s = edit(s, kind)
    if i % 10 == 3:
        at = rng.randrange(MARGIN, len(s) - MARGIN)
        s = s[:at] + "N" + s[at + 1:]
    out.append(">r%d_%s_%d%s_%s\n%s\n" % (i, g_name, st, strand, "".join(kinds) or "0", s))
out.append(">random\n%s\n" % "".join(rng.choice("ACGT") for _ in range(90)))
open(os.path.join(GOLDEN, "sw_reads.fa"), "w").write("".join(out))


def lines_of(fn):
    return gzip.open(os.path.join(GOLDEN, fn), "rt").read().split()


runs = []
c = lines_of("copies3000.txt.gz")[0]
runs += [c[:90], c[100:140] + ("A" if c[140] != "A" else "C") + c[141:190], c[300:340]]
for l in lines_of("longruns.txt.gz"):
    runs += [l[:60], l[len(l) // 2:len(l) // 2 + 45]]
runs.append("A" * 45)
open(os.path.join(GOLDEN, "sw_runs.txt"), "w").write("".join(r + "\n" for r in runs))
