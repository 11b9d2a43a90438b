#!/usr/bin/env python3
"""mem at scale: builds a seeded index with the CLI (K relatives of an L bp genome, tools/gen_family.py; both strands: 2 K L symbols),
makes two query sets -- (a) N simulated 150 bp reads of the base genome with 1 % errors, (b) one further relative as a single record --
and runs `ropebwt3-amd mem -l31` and the reference's `mem` (-t1 and -t16) on each, every run under a timeout.  One JSON line: wall times
(warm-up + --runs runs of the CLI: median, min, max), whether the md5 of the outputs match, extension steps, the walkers' kernel time
and steps per second (the CLI's -v3 line), and for (b) the wall and kernel time per --chunk, one walker for the whole query included.
    python tools/probe_mem.py [--K 8] [--L 4000000] [--reads 2000000] [--runs 3] [--workdir DIR] [--ref-timeout 300] [--skip-t1]"""
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

LINE = re.compile(rb"(\d+) queries in (\d+) batch\(es\): (\d+) matches from (\d+) walkers in (\d+) slice\(s\), (\d+) extensions; ([\d.]+) ms in the engine, walkers' kernel ([\d.]+) ms")


def write_reads(fn, g0, n, rng):
    pos = rng.integers(0, g0.size - 150, size=n)
    with open(fn, "wb") as f:
        for lo in range(0, n, 100000):
            p = pos[lo:lo + 100000]
            r = g0[p[:, None] + np.arange(150)[None, :]]
            m = rng.random(r.shape) < 0.01
            r[m] = gen_family.ALPH[rng.integers(0, 4, size=int(m.sum()))]
            rows = np.concatenate([np.full((p.size, 1), ord("\n"), dtype=np.uint8), r, np.full((p.size, 1), ord("\n"), dtype=np.uint8)], axis=1)
            for i in range(p.size):
                f.write(b">r%d" % (lo + i))
                f.write(rows[i].tobytes())


def cli_run(args, timeout, runs):
    env = dict(os.environ, RB3_VERBOSE="3")
    walls, last = [], None
    for i in range(runs + 1):   # the first run is the warm-up
        last = run_md5([CLI, "mem"] + args, timeout, env)
        if last[0] is None or last[1] != 0:
            break
        if i > 0:
            walls.append(last[0])
    wall, rc, md5, lines, err = last
    out = {"rc": rc, "md5": md5, "lines": lines, "timed_out": wall is None}
    if walls:
        out.update({"wall_s_median": round(statistics.median(walls), 3), "wall_s_min": round(min(walls), 3), "wall_s_max": round(max(walls), 3), "runs": len(walls)})
    m = LINE.search(err or b"")
    if m:
        steps, ms_eng, ms_walk = int(m[6]), float(m[7]), float(m[8])
        out.update({"queries": int(m[1]), "matches": int(m[3]), "walkers": int(m[4]), "slices": int(m[5]), "steps": steps, "ms_engine": ms_eng, "ms_walk": ms_walk,
                    "steps_per_s_kernel": round(steps / (ms_walk * 1e-3)) if ms_walk > 0 else None})
    return out


def ref_run(args, threads, timeout):
    wall, rc, md5, lines, _ = run_md5([REF, "mem", "-t%d" % threads] + args, timeout)
    return {"wall_s": round(wall, 3) if wall else None, "rc": rc, "md5": md5, "timed_out": wall is None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--l", type=int, default=31)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunks", default="256,1024,2048,4096,16384,131072")
    ap.add_argument("--workdir", default="/tmp/rb3_mem_probe")
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--ref-timeout", type=float, default=300)
    ap.add_argument("--skip-t1", action="store_true")
    ap.add_argument("--no-whole", action="store_true", help="skip (b) with one walker for the whole query")
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, idx = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd")
    qa, qb = os.path.join(a.workdir, "reads.fa"), os.path.join(a.workdir, "contig.fa")
    t = time.time()
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    t_build = time.time() - t
    g0 = gen_family.ALPH[np.random.default_rng(11).integers(0, 4, size=a.L)]   # (the base genome of gen_family.relatives)
    write_reads(qa, g0, a.reads, np.random.default_rng(31))
    with open(qb, "wb") as f:
        gen_family._fasta(f, "relative_x", gen_family._mutate(g0, np.random.default_rng(999), 0.001))
    out = {"probe": "mem", "K": a.K, "L": a.L, "l": a.l, "n_symbols": 2 * a.K * a.L, "reads": a.reads, "seconds_build_cli": round(t_build, 2)}
    for tag, q in (("a_reads", qa), ("b_contig", qb)):
        args = ["-l%d" % a.l, idx, q]
        g = cli_run(args, a.timeout, a.runs)
        out[tag] = {"gpu": g}
        if os.path.exists(REF):
            for th in ([16] if a.skip_t1 else [16, 1]):
                r = ref_run(args, th, a.ref_timeout)
                r["md5_match"] = r["md5"] == g["md5"] if r["md5"] else None
                if r["wall_s"] and g.get("wall_s_median"):
                    r["speedup"] = round(r["wall_s"] / g["wall_s_median"], 1)
                out[tag]["ref_t%d" % th] = r
        print(json.dumps({tag: out[tag]}), file=sys.stderr, flush=True)
    sweep = {}
    for c in [int(x) for x in a.chunks.split(",")] + ([] if a.no_whole else [2 ** 31 - 1]):
        g = cli_run(["--chunk", str(c), "-l%d" % a.l, idx, qb], a.timeout, 1)
        sweep[str(c)] = {k: g.get(k) for k in ("wall_s_median", "ms_walk", "ms_engine", "steps", "walkers", "md5", "timed_out")}
        sweep[str(c)]["md5_match"] = g["md5"] == out["b_contig"]["gpu"]["md5"]
    out["b_chunk_sweep"] = sweep
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
