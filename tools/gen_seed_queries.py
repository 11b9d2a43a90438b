#!/usr/bin/env python3
"""The lines of the `sw --prefilter` goldens, tests/golden/seed_lines.txt: one query per line (-L), made from tests/golden/genomes12.fa.gz
with a fixed seed, of the kinds that the MEM pre-filter of `sw -j` tells apart at -j20 and -j30:
  exact substrings of both strands; foreign random lines; lines with substitutions placed so that the longest stretch that occurs in the
  index, on either strand, is exactly 19, 20, 29 and 30 symbols (checked here against both strands of every genome; a substitution that
  happens to match elsewhere is drawn again); a line of only N; lines shorter than 20; an empty line between two others; and a foreign
  line directly in front of an exact one, so that a filtered query stands in front of a query with a hit.
Lines are 20 to 300 symbols unless their kind says otherwise.
    python tools/gen_seed_queries.py"""
import gzip, os, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 20260308
COMP = str.maketrans("ACGT", "TGCA")

rng = random.Random(SEED)
genomes = []
for line in gzip.open(os.path.join(GOLDEN, "genomes12.fa.gz"), "rt"):
    if line.startswith(">"):
        genomes.append([])
    else:
        genomes[-1].append(line.strip().upper())
genomes = ["".join(g) for g in genomes]
both = genomes + [g.translate(COMP)[::-1] for g in genomes]


def longest(s):
    """the longest stretch of s that occurs in a genome, on either strand"""
    best = 0
    for x in range(len(s)):
        while x + best < len(s) and any(s[x:x + best + 1] in g for g in both):
            best += 1
    return best


def piece(length):
    g = genomes[rng.randrange(len(genomes))]
    st = rng.randrange(0, len(g) - length)
    return g[st:st + length]


def rc(s):
    return s.translate(COMP)[::-1]


def foreign(length):
    while True:
        s = "".join(rng.choice("ACGT") for _ in range(length))
        if longest(s) < 19:
            return s


def stretches(target, n_stretch, flip):
    """n_stretch stretches of `target` symbols of a genome with one substituted symbol between neighbours: the longest stretch that occurs is `target`"""
    while True:
        s = list(piece(n_stretch * target + n_stretch - 1))
        for i in range(1, n_stretch):
            at = i * target + i - 1
            s[at] = rng.choice([c for c in "ACGT" if c != s[at]])
        s = "".join(s)
        if longest(s) == target:
            return rc(s) if flip else s


lines = []
for i in range(6):                                   # exact, both strands
    s = piece(rng.choice((20, 31, 60, 150, 300, 77)))
    lines.append(rc(s) if i % 2 else s)
lines.append(foreign(120))                           # a filtered line in front of a line with a hit
lines.append(piece(90))
for length in (20, 45, 200, 300):
    lines.append(foreign(length))
for target in (19, 20, 29, 30):                      # just below and just at -j20 and -j30
    for k, n in enumerate((3, 4, 6)):
        lines.append(stretches(target, n, k % 2 == 1))
lines.append("N" * 40)
lines.append(piece(19))                              # shorter than 20
lines.append(piece(8))
lines.append(piece(64))
lines.append("")                                     # an empty line between two others
lines.append(rc(piece(64)))
lines.append(foreign(70) + piece(25) + foreign(60))  # a seed in the middle of a foreign line
p45 = piece(45)
lines.append(p45[:22] + "N" + p45[23:])              # an N of the query between two stretches of 22 symbols that occur
lines.append(foreign(33))
lines.append(piece(120))
assert all(len(l) <= 300 for l in lines)
open(os.path.join(GOLDEN, "seed_lines.txt"), "w").write("".join(l + "\n" for l in lines))
print("%d lines" % len(lines))
