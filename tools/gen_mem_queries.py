#!/usr/bin/env python3
"""The two query fixtures of the `mem` tests, seeded (plain data made here, not by the reference):
  tests/golden/mem_mutated.fa.gz  the first two records of genomes12_part1.fa.gz with about 1 % substitutions, 0.2 % deletions and
                                  0.2 % insertions (some of them N), lines of 70 with every second line in lower case, a comment after the name
  tests/golden/mem_iupac.fa       records with IUPAC codes, an empty record, a record shorter than -l19, a name without a comment, and records that
                                  match in the other committed indexes (copies3000, longruns, reads_fq)
    python tools/gen_mem_queries.py"""
import gzip, os, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fasta(path):
    name, seq, out = None, [], []
    for line in gzip.open(path, "rt"):
        line = line.rstrip("\n")
        if line.startswith(">"):
            if name is not None:
                out.append((name, "".join(seq)))
            name, seq = line[1:].split()[0], []
        else:
            seq.append(line)
    if name is not None:
        out.append((name, "".join(seq)))
    return out


def fasta_first_read(path):
    """the sequence of the first record of a FASTA / FASTQ file"""
    with gzip.open(path, "rt") as f:
        f.readline()
        return f.readline().strip()


def mutate(rng, s):
    out = []
    for ch in s:
        r = rng.random()
        if r < 0.002:
            continue                                   # deletion
        if r < 0.004:
            out.append(rng.choice("ACGTN"))            # insertion
        if r < 0.014:
            ch = rng.choice([c for c in "ACGT" if c != ch.upper()])
        out.append(ch)
    return "".join(out)


def main():
    rng = random.Random(20240607)
    recs = fasta(os.path.join(GOLDEN, "genomes12_part1.fa.gz"))[:2]
    lines = []
    for i, (name, seq) in enumerate(recs):
        m = mutate(rng, seq.upper())
        lines.append(">%s_mut%d about 1%% substitutions, 0.2%% deletions, 0.2%% insertions" % (name, i + 1))
        for k in range(0, len(m), 70):
            lines.append(m[k:k + 70].lower() if (k // 70) & 1 else m[k:k + 70])
    with open(os.path.join(GOLDEN, "mem_mutated.fa.gz"), "wb") as f:
        with gzip.GzipFile(filename="", fileobj=f, mode="wb", mtime=0) as g:
            g.write(("\n".join(lines) + "\n").encode())
    src = recs[0][1].upper()
    iupac = list(src[1000:1400])
    for k in range(30, 400, 41):
        iupac[k] = "RYKMSWBDHVN"[(k // 41) % 11]
    with open(os.path.join(GOLDEN, "mem_iupac.fa"), "w") as f:
        f.write(">iupac codes of every kind\n%s\n" % "".join(iupac))
        f.write(">empty\n")
        f.write(">short\tshorter than -l19\n%s\n" % src[5000:5012])
        f.write(">nocomment\n%s\n%s\n" % (src[7000:7100].lower(), src[7100:7160]))
        f.write(">allN\n%s\n" % ("N" * 25))
        f.write(">exact400 a stretch without a change\n%s\n" % src[20000:20400])
        copy = gzip.open(os.path.join(GOLDEN, "copies3000.txt.gz"), "rt").readline().strip()
        f.write(">copy of copies3000 with one change\n%s\n" % (copy[:260] + "N" + copy[261:]))
        f.write(">polyA\n%s\n" % ("A" * 320 + "C" + "T" * 230))
        read = fasta_first_read(os.path.join(GOLDEN, "reads_fq.fa.gz"))
        f.write(">read of reads_fq\n%s\n" % read)


if __name__ == "__main__":
    main()
