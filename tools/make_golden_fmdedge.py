#!/usr/bin/env python3
"""tests/golden/FMDEDGE_MANIFEST.json: size, word count and md5 of the .fmd data section the UNMODIFIED reference
(oracle/_ref/ropebwt3 plain2fmd, built by oracle/Makefile) writes for the four superblock cases of tests/fmd_cases.py -- BWTs of
10^8 runs whose .fmd crosses, meets or stops one block short of the border of a superblock of 2^20 blocks.  Only the md5s are
kept: each data section is 64 MiB.  Run once where the reference sources are present."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fmd_cases as C  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/ropebwt3 is not built")
    man = {}
    with tempfile.TemporaryDirectory() as d:
        for case in sorted(C.SUPER):
            src, out = os.path.join(d, case + ".txt"), os.path.join(d, case + ".fmd")
            np.frombuffer(b"$ACGTN", dtype=np.uint8)[C.super_plain(case)].tofile(src)
            subprocess.run([REF, "plain2fmd", "-o", out, src], stderr=subprocess.DEVNULL, check=True)
            words, mcnt = C.fmd_data_words(np.fromfile(out, dtype=np.uint8))
            man[case] = {"n_runs": C.SUPER[case], "n_symbols": int(mcnt.sum()), "data_bytes": int(words.nbytes), "n_words": int(words.size),
                         "data_md5": hashlib.md5(words.tobytes()).hexdigest(), "cmd": "plain2fmd %s.txt" % case}
            os.remove(src), os.remove(out)
    json.dump(man, open(os.path.join(GOLDEN, "FMDEDGE_MANIFEST.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(man, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
