#!/usr/bin/env python3
"""BRE fixtures from the UNMODIFIED reference (oracle/_ref/ropebwt3, built by oracle/Makefile): tests/golden/BRE_MANIFEST.json
with size and md5 of `build -e -i X.fmd` for every committed .fmd and of `build -e` from sequence files, and the small files
themselves (tests/golden/*.bre).  Run once where the reference sources are present."""
import glob
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")
KEEP = ("k4_readme", "k2_fwd", "edge_chars", "edge_dups", "longruns", "copies3000")   # committed as files; the rest by md5


def ref(args):
    return subprocess.run([REF] + args, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout


def entry(data, cmd):
    n_rec, n_sym, n_run = (int.from_bytes(data[len(data) - 24 + 8 * i:len(data) - 16 + 8 * i], "little") for i in range(3))
    return {"bytes": len(data), "md5": hashlib.md5(data).hexdigest(), "n_rec": n_rec, "n_sym": n_sym, "n_run": n_run, "cmd": cmd}


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/ropebwt3 is not built")
    man = {"from_fmd": {}, "from_seq": {}}
    for fmd in sorted(glob.glob(os.path.join(GOLDEN, "*.fmd"))):
        name = os.path.basename(fmd)[:-4]
        data = ref(["build", "-e", "-i", fmd])
        man["from_fmd"][name] = entry(data, "build -e -i %s.fmd" % name)
        if name in KEEP:
            open(os.path.join(GOLDEN, name + ".bre"), "wb").write(data)
            man["from_fmd"][name]["file"] = name + ".bre"
    g = lambda f: os.path.join(GOLDEN, f)
    for key, flags, inp in (("genomes12", [], "genomes12.fa.gz"), ("reads_fq_rclo", ["-r"], "reads_fq.fa.gz"), ("reads_fq_rlo", ["-s"], "reads_fq.fa.gz"),
                            ("reads_fq", [], "reads_fq.fa.gz"), ("genomes12_F", ["-F"], "genomes12.fa.gz"), ("genomes12_R", ["-R"], "genomes12.fa.gz")):
        e = entry(ref(["build", "-e"] + flags + [g(inp)]), "build -e %s %s" % (" ".join(flags), inp))
        e["flags"], e["input"] = flags, inp
        man["from_seq"][key] = e
    json.dump(man, open(os.path.join(GOLDEN, "BRE_MANIFEST.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(man, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
