#!/usr/bin/env python3
"""hapdiv at scale: the seeded index of tools/probe_mem.py (K relatives of an L bp genome, both strands: 2 K L symbols), one further
relative as a single L bp query, `ropebwt3-amd hapdiv` at the defaults and the reference's `hapdiv` at -t16 and -t1, every run under
a timeout of its own (run_md5 of tools/probe_kount.py) and none started after one that did not end normally.  Writes
profiles/hapdiv_probe.json and prints it: wall times (a warm-up + --runs runs of the CLI: median, min, max), the engine call, the
DP kernel (HIP events), extensions and extensions per second, the share of windows whose table went to global memory (the CLI's -v3
line), the reference's wall times and whether the md5 of the outputs match.
    python tools/probe_hapdiv.py [--K 8] [--L 4000000] [--runs 3] [--workdir DIR] [--ref-timeout 600] [--skip-t1]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_family  # noqa: E402
from tools.probe_kount import run_md5, CLI, REF  # noqa: E402

LINE = re.compile(rb"(\d+) queries in (\d+) batch\(es\): (\d+) windows in (\d+) slice\(s\), (\d+) extensions, (\d+) windows with a table in global memory; ([\d.]+) ms in the engine, the DP kernel ([\d.]+) ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_hapdiv_probe")
    ap.add_argument("--timeout", type=float, default=300)
    ap.add_argument("--ref-timeout", type=float, default=600)
    ap.add_argument("--skip-t1", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, idx, q = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd"), os.path.join(a.workdir, "contig.fa")
    t = time.time()
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    t_build = time.time() - t
    g0 = gen_family.ALPH[np.random.default_rng(11).integers(0, 4, size=a.L)]   # (the base genome of gen_family.relatives)
    with open(q, "wb") as f:
        gen_family._fasta(f, "relative_x", gen_family._mutate(g0, np.random.default_rng(999), 0.001))
    out = {"probe": "hapdiv", "K": a.K, "L": a.L, "n_symbols": 2 * a.K * a.L, "seconds_build_cli": round(t_build, 2)}
    env = dict(os.environ, RB3_VERBOSE="3")
    walls, last = [], None
    for i in range(a.runs + 1):   # the first run is the warm-up
        last = run_md5([CLI, "hapdiv", idx, q], a.timeout, env)
        if last[0] is None or last[1] != 0:
            break
        if i > 0:
            walls.append(last[0])
    wall, rc, md5, lines, err = last
    g = {"rc": rc, "md5": md5, "lines": lines, "timed_out": wall is None}
    if walls:
        g.update({"wall_s_median": round(statistics.median(walls), 3), "wall_s_min": round(min(walls), 3), "wall_s_max": round(max(walls), 3), "runs": len(walls)})
    m = LINE.search(err or b"")
    if m:
        n_win, n_ext, n_t2, ms_eng, ms_dp = int(m[3]), int(m[5]), int(m[6]), float(m[7]), float(m[8])
        g.update({"windows": n_win, "slices": int(m[4]), "extensions": n_ext, "share_global_table": round(n_t2 / n_win, 4) if n_win else None, "ms_engine": ms_eng,
                  "ms_dp": ms_dp, "extensions_per_s_kernel": round(n_ext / (ms_dp * 1e-3)) if ms_dp > 0 else None})
    out["gpu"] = g
    if rc == 0 and wall is not None and os.path.exists(REF):   # (nothing more after a run that did not end normally)
        for th in ([16] if a.skip_t1 else [16, 1]):
            w, r, rmd5, _, _ = run_md5([REF, "hapdiv", "-t%d" % th, idx, q], a.ref_timeout)
            e = {"wall_s": round(w, 3) if w else None, "rc": r, "md5": rmd5, "timed_out": w is None, "md5_match": rmd5 == md5 if rmd5 else None}
            if w and g.get("wall_s_median"):
                e["speedup"] = round(w / g["wall_s_median"], 2)
            out["ref_t%d" % th] = e
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "hapdiv_probe.json"), "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
