#!/usr/bin/env python3
"""mem -p at scale, on workload (a) of tools/probe_mem.py: a seeded index built with the CLI (K relatives of an L bp genome, both strands),
its sampled suffix array (`ropebwt3-amd ssa -s8`) and name list beside it, N simulated 150 bp reads with 1 % errors; `mem -l31` with and
without `-p10` here and in the reference (-t16, -t1), every run under a timeout.  One JSON line: wall times (warm-up + --runs runs: median,
min, max), whether the md5 of the outputs match, the locate kernels' time, heap pops and pops per second beside the walkers' steps per
second (the CLI's -v3 lines), the share of matches that took a heap in global memory, the largest heap, and what -p10 costs over plain mem
on either side.
    python tools/probe_mempos.py [--K 8] [--L 4000000] [--reads 2000000] [--p 10] [--s 8] [--runs 3] [--workdir DIR] [--skip-t1]"""
import argparse
import gzip
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_family  # noqa: E402
from tools.probe_kount import CLI, REF  # noqa: E402
from tools.probe_mem import cli_run, ref_run, write_reads  # noqa: E402

LOC = re.compile(rb"(\d+) positions of (\d+) matches: (\d+) heap pops, (\d+) matches with a heap in global memory, largest heap (\d+); locate kernels ([\d.]+) ms")


def cli_pos_run(args, timeout, runs):
    """cli_run plus the locate line of -v3 (one more run: cli_run keeps the text of its last run to itself)"""
    out = cli_run(args, timeout, runs)
    r = subprocess.run([CLI, "mem"] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout, env=dict(os.environ, RB3_VERBOSE="3"))
    m = LOC.search(r.stderr)
    if m:
        pairs, n, pops, t2, top, ms = int(m[1]), int(m[2]), int(m[3]), int(m[4]), int(m[5]), float(m[6])
        out.update({"positions": pairs, "located": n, "pops": pops, "tier2": t2, "tier2_share": round(t2 / n, 6) if n else None, "max_heap": top, "ms_locate": ms,
                    "pops_per_s_kernel": round(pops / (ms * 1e-3)) if ms > 0 else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--l", type=int, default=31)
    ap.add_argument("--p", type=int, default=10)
    ap.add_argument("--s", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_mempos_probe")
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--ref-timeout", type=float, default=300)
    ap.add_argument("--skip-t1", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, idx, qa = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd"), os.path.join(a.workdir, "reads.fa")
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    t = time.time()
    subprocess.run([CLI, "ssa", "-s%d" % a.s, "-o", idx + ".ssa", idx], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    t_ssa = time.time() - t
    with gzip.open(idx + ".len.gz", "wt") as f:   # the one-line recipe of the README: name and length of every record
        name, n = None, 0
        for line in open(fa):
            if line[0] == ">":
                if name is not None:
                    f.write("%s\t%d\n" % (name, n))
                name, n = line[1:].split()[0], 0
            else:
                n += len(line.strip())
        f.write("%s\t%d\n" % (name, n))
    g0 = gen_family.ALPH[np.random.default_rng(11).integers(0, 4, size=a.L)]
    write_reads(qa, g0, a.reads, np.random.default_rng(31))
    out = {"probe": "mempos", "K": a.K, "L": a.L, "l": a.l, "p": a.p, "s": a.s, "n_symbols": 2 * a.K * a.L, "reads": a.reads, "seconds_ssa_cli": round(t_ssa, 2)}
    for tag, extra in (("plain", []), ("pos", ["-p%d" % a.p])):
        args = ["-l%d" % a.l] + extra + [idx, qa]
        g = cli_pos_run(args, a.timeout, a.runs) if extra else cli_run(args, a.timeout, a.runs)
        out[tag] = {"gpu": g}
        if os.path.exists(REF):
            for th in ([16] if a.skip_t1 else [16, 1]):
                r = ref_run(args, th, a.ref_timeout)
                r["md5_match"] = r["md5"] == g["md5"] if r["md5"] else None
                if r["wall_s"] and g.get("wall_s_median"):
                    r["speedup"] = round(r["wall_s"] / g["wall_s_median"], 1)
                out[tag]["ref_t%d" % th] = r
        print(json.dumps({tag: out[tag]}), file=sys.stderr, flush=True)
    try:
        out["cost_of_p_gpu_s"] = round(out["pos"]["gpu"]["wall_s_median"] - out["plain"]["gpu"]["wall_s_median"], 3)
        out["cost_of_p_ref_t16_s"] = round(out["pos"]["ref_t16"]["wall_s"] - out["plain"]["ref_t16"]["wall_s"], 3)
    except (KeyError, TypeError):
        pass
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
