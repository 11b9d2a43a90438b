#!/usr/bin/env python3
"""sw --local at scale: the index, name list, sampled suffix array and simulated reads of tools/probe_sw.py (K relatives of an L bp genome,
both strands; --reads 150 bp reads of a further relative with 1 % errors, half of them reverse-complemented), `ropebwt3-amd sw --local -p1`
and the reference's `sw -p1` at -t16 and -t1, every run under a timeout of its own (run_md5 of tools/probe_kount.py) and none started
after one that did not end normally.  Writes profiles/swlocal_probe.json and prints it: wall times (a warm-up + --runs runs of the CLI:
median, min, max), the engine call, the DP kernel, the backtrack kernel and the locate kernels (HIP events), the host's time for the
graphs of the queries, their nodes and edges, extensions and extensions per second, the reference's wall times and whether the md5 of the
outputs match.
    python tools/probe_swlocal.py [--K 8] [--L 4000000] [--reads 1000000] [--runs 3] [--workdir DIR] [--ref-timeout 900] [--skip-t1]"""
import argparse
import gzip
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
from tools.probe_sw import LINE, simulate  # noqa: E402

GRAPHS = re.compile(rb"the graphs: (\d+) nodes, (\d+) edges, ([\d.]+) ms on the host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_swlocal_probe")
    ap.add_argument("--timeout", type=float, default=600)
    ap.add_argument("--ref-timeout", type=float, default=900)
    ap.add_argument("--skip-t1", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, idx, q = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd"), os.path.join(a.workdir, "reads.fa")
    t = time.time()
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    subprocess.run([CLI, "ssa", "-s8", "-o", idx + ".ssa", idx], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    recs = []
    for l in open(fa):
        if l.startswith(">"):
            recs.append([l[1:].split()[0], 0])
        else:
            recs[-1][1] += len(l.strip())
    with gzip.open(idx + ".len.gz", "wt") as f:
        f.write("".join("%s\t%d\n" % (n, ln) for n, ln in recs))
    t_build = time.time() - t
    g0 = gen_family.ALPH[np.random.default_rng(11).integers(0, 4, size=a.L)]   # (the base genome of gen_family.relatives)
    rel = gen_family._mutate(g0, np.random.default_rng(999), 0.001)
    simulate(bytes(rel), a.reads, 150, 0.01, np.random.default_rng(7), q)
    out = {"probe": "swlocal", "K": a.K, "L": a.L, "n_symbols": 2 * a.K * a.L, "reads": a.reads, "read_len": 150, "err": 0.01, "opts": "--local -p1", "seconds_build_cli": round(t_build, 2)}
    env = dict(os.environ, RB3_VERBOSE="3")
    walls, last = [], None
    for i in range(a.runs + 1):   # the first run is the warm-up
        last = run_md5([CLI, "sw", "--local", "-p1", idx, q], a.timeout, env)
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
        n_ext, ms_dp = int(m[5]), float(m[8])
        g.update({"hits": int(m[3]), "slices": int(m[4]), "extensions": n_ext, "queries_global_table": int(m[6]), "ms_engine": float(m[7]), "ms_dp": ms_dp,
                  "ms_backtrack": float(m[9]), "ms_locate": float(m[10]), "extensions_per_s_kernel": round(n_ext / (ms_dp * 1e-3)) if ms_dp > 0 else None})
    m = GRAPHS.search(err or b"")
    if m:
        g.update({"nodes": int(m[1]), "edges": int(m[2]), "ms_dawg_host": float(m[3])})
    out["gpu"] = g
    if rc == 0 and wall is not None and os.path.exists(REF):   # (nothing more after a run that did not end normally)
        for th in ([16] if a.skip_t1 else [16, 1]):
            w, r, rmd5, _, _ = run_md5([REF, "sw", "-p1", "-t%d" % th, idx, q], a.ref_timeout)
            e = {"wall_s": round(w, 3) if w else None, "rc": r, "md5": rmd5, "timed_out": w is None, "md5_match": rmd5 == md5 if rmd5 else None}
            if w and g.get("wall_s_median"):
                e["speedup"] = round(w / g["wall_s_median"], 2)
            out["ref_t%d" % th] = e
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "swlocal_probe.json"), "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
