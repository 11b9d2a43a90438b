#!/usr/bin/env python3
"""sw --prefilter at scale: the index, name list and sampled suffix array of tools/probe_sw.py (K relatives of an L bp genome, both strands)
and its simulated reads (--reads 150 bp reads of a further relative with 1 % errors), every second read replaced by a foreign one (uniform
random symbols of the same length): half of the batch has nothing to align.  Times `ropebwt3-amd sw -e --prefilter -j20 -p1` against
`sw -e -p1`, and `sw --local --prefilter -j20 -p1` against `sw --local -p1` (a warm-up + --runs runs each: median, min, max), then the
reference's `sw -e -j20 -p1` and `sw -j20 -p1` at -t16, every run under a timeout of its own (run_md5 of tools/probe_kount.py) and none
started after one that did not end normally.  Writes profiles/swseed_probe.json and prints it: wall times, the engine's time, the seed
kernel's time (ms_walk), its walkers, steps and steps per second -- beside the 7.5 G steps/s of k_suffix_walk in profiles/walk_probe.json
--, the queries filtered, and whether the md5 of the filtered outputs match the reference's.
    python tools/probe_swseed.py [--K 8] [--L 4000000] [--reads 200000] [--runs 3] [--workdir DIR] [--ref-timeout 600]"""
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

SEED = re.compile(rb"the pre-filter: (\d+) queries without a seed of (\d+) symbols were not aligned; (\d+) walkers, (\d+) extension steps, the seed kernel ([\d.]+) ms")


def half_foreign(fn, rng):
    """every second record of a FASTA file of one-line records gets random symbols of the same length"""
    ls = open(fn, "rb").read().split(b"\n")
    n = 0
    for i in range(1, len(ls), 2):
        if (i >> 1) & 1 and ls[i]:
            ls[i] = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=len(ls[i])))
            n += 1
    open(fn, "wb").write(b"\n".join(ls))
    return n


def timed(cmd, runs, timeout, env):
    walls, last = [], None
    for i in range(runs + 1):   # the first run is the warm-up
        last = run_md5(cmd, timeout, env)
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
        g.update({"hits": int(m[3]), "extensions": int(m[5]), "ms_engine": float(m[7]), "ms_dp": float(m[8]), "ms_backtrack": float(m[9]), "ms_locate": float(m[10])})
    m = SEED.search(err or b"")
    if m:
        steps, ms = int(m[4]), float(m[5])
        g.update({"filtered": int(m[1]), "walkers": int(m[3]), "steps": steps, "ms_walk": ms, "steps_per_s_kernel": round(steps / (ms * 1e-3)) if ms > 0 else None})
    return g, rc == 0 and wall is not None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_swseed_probe")
    ap.add_argument("--timeout", type=float, default=600)
    ap.add_argument("--ref-timeout", type=float, default=600)
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
    n_foreign = half_foreign(q, np.random.default_rng(8))
    out = {"probe": "swseed", "K": a.K, "L": a.L, "n_symbols": 2 * a.K * a.L, "reads": a.reads, "foreign": n_foreign, "read_len": 150, "err": 0.01, "min_mem_len": 20,
           "seconds_build_cli": round(t_build, 2), "k_suffix_walk_steps_per_s": 7507513607}
    env = dict(os.environ, RB3_VERBOSE="3")
    ok = True
    for name, mode, ref_mode in (("e2e", ["-e"], ["-e"]), ("local", ["--local"], [])):
        for tag, extra in (("filtered", ["--prefilter", "-j20"]), ("unfiltered", [])):
            if ok:
                out["%s_%s" % (name, tag)], ok = timed([CLI, "sw"] + mode + extra + ["-p1", idx, q], a.runs, a.timeout, env)
        f, u = out.get(name + "_filtered", {}), out.get(name + "_unfiltered", {})
        if f.get("wall_s_median") and u.get("wall_s_median"):
            out[name + "_speedup_wall"] = round(u["wall_s_median"] / f["wall_s_median"], 2)
            if f.get("ms_engine") and u.get("ms_engine"):
                out[name + "_speedup_engine"] = round(u["ms_engine"] / f["ms_engine"], 2)
        if ok and os.path.exists(REF):   # (nothing more after a run that did not end normally)
            w, r, rmd5, _, _ = run_md5([REF, "sw"] + ref_mode + ["-j20", "-p1", "-t16", idx, q], a.ref_timeout)
            e = {"wall_s": round(w, 3) if w else None, "rc": r, "md5": rmd5, "timed_out": w is None, "md5_match": rmd5 == f.get("md5") if rmd5 else None}
            if w and f.get("wall_s_median"):
                e["speedup"] = round(w / f["wall_s_median"], 2)
            out[name + "_ref_t16"] = e
            ok = w is not None and r == 0
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "swseed_probe.json"), "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
