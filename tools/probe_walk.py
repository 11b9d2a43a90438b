#!/usr/bin/env python3
"""suffix and get at scale: (a) builds the seeded index of tools/probe_mem.py with the CLI (K relatives of an L bp genome, both strands: 2 K L
symbols), makes N simulated 150 bp reads of the base genome with 1 % errors and runs `ropebwt3-amd suffix` and the reference's `suffix` (which
has no threads option: one thread) on them; (b) builds an index of R such reads and runs `ropebwt3-amd get 0 .. R - 1` and the reference's `get`.
Every run under a timeout.  One JSON document, written to --out as well: wall times (warm-up + --runs runs of the CLI: median, min, max), whether
the md5 of the outputs match, steps, kernel times and steps per second (the CLI's -v3 lines).
    python tools/probe_walk.py [--K 8] [--L 4000000] [--reads 1000000] [--rows 10000] [--runs 3] [--workdir DIR] [--out profiles/walk_probe.json]"""
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
from tools.probe_mem import write_reads  # noqa: E402

SUFFIX_LINE = re.compile(rb"(\d+) queries of (\d+) symbols in (\d+) batch\(es\) and (\d+) slice\(s\): (\d+) extensions; ([\d.]+) ms in the engine, walk kernel ([\d.]+) ms")
GET_LINE = re.compile(rb"(\d+) rows, (\d+) symbols in (\d+) slice\(s\): (\d+) LF steps; ([\d.]+) ms in the engine, counting walk ([\d.]+) ms, writing walk ([\d.]+) ms")


def cli_run(cmd, args, timeout, runs):
    env = dict(os.environ, RB3_VERBOSE="3")
    walls, last = [], None
    for i in range(runs + 1):   # the first run is the warm-up
        last = run_md5([CLI, cmd] + args, timeout, env)
        if last[0] is None or last[1] != 0:
            break
        if i > 0:
            walls.append(last[0])
    wall, rc, md5, lines, err = last
    out = {"rc": rc, "md5": md5, "lines": lines, "timed_out": wall is None}
    if walls:
        out.update({"wall_s_median": round(statistics.median(walls), 3), "wall_s_min": round(min(walls), 3), "wall_s_max": round(max(walls), 3), "runs": len(walls)})
    if cmd == "suffix":
        m = SUFFIX_LINE.search(err or b"")
        if m:
            steps, ms_walk = int(m[5]), float(m[7])
            out.update({"queries": int(m[1]), "symbols": int(m[2]), "slices": int(m[4]), "steps": steps, "ms_engine": float(m[6]), "ms_walk": ms_walk,
                        "steps_per_s_kernel": round(steps / (ms_walk * 1e-3)) if ms_walk > 0 else None})
    else:
        m = GET_LINE.search(err or b"")
        if m:
            steps, ms_count, ms_emit = int(m[4]), float(m[6]), float(m[7])
            out.update({"rows": int(m[1]), "symbols": int(m[2]), "slices": int(m[3]), "steps": steps, "ms_engine": float(m[5]), "ms_count": ms_count, "ms_emit": ms_emit,
                        "steps_per_s_kernel": round(steps / ((ms_count + ms_emit) * 1e-3)) if ms_count + ms_emit > 0 else None})
    return out


def ref_run(cmd, args, timeout, g):
    wall, rc, md5, lines, _ = run_md5([REF, cmd] + args, timeout)
    r = {"wall_s": round(wall, 3) if wall else None, "rc": rc, "md5": md5, "timed_out": wall is None, "threads": 1}
    r["md5_match"] = r["md5"] == g["md5"] if r["md5"] else None
    if r["wall_s"] and g.get("wall_s_median"):
        r["speedup"] = round(r["wall_s"] / g["wall_s_median"], 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_walk_probe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_probe.json"))
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--ref-timeout", type=float, default=300)
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, idx = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd")
    qa, fb, idxb = os.path.join(a.workdir, "reads.fa"), os.path.join(a.workdir, "reads10k.fa"), os.path.join(a.workdir, "reads10k.fmd")
    t = time.time()
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    t_build = time.time() - t
    g0 = gen_family.ALPH[np.random.default_rng(11).integers(0, 4, size=a.L)]   # (the base genome of gen_family.relatives)
    write_reads(qa, g0, a.reads, np.random.default_rng(31))
    write_reads(fb, g0, a.rows, np.random.default_rng(32))
    subprocess.run([CLI, "build", "-d", "-o", idxb, fb], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    out = {"probe": "walk", "K": a.K, "L": a.L, "n_symbols": 2 * a.K * a.L, "reads": a.reads, "rows": a.rows, "seconds_build_cli": round(t_build, 2)}
    for tag, cmd, args in (("a_suffix", "suffix", [idx, qa]), ("b_get", "get", [idxb] + [str(i) for i in range(a.rows)])):
        g = cli_run(cmd, args, a.timeout, a.runs)
        out[tag] = {"gpu": g}
        if os.path.exists(REF):
            out[tag]["ref_t1"] = ref_run(cmd, args, a.ref_timeout, g)
        print(json.dumps({tag: out[tag]}), file=sys.stderr, flush=True)
    mem = os.path.join(ROOT, "profiles", "mem_probe_1m_reads.json")
    if os.path.exists(mem) and out["a_suffix"]["gpu"].get("steps_per_s_kernel"):   # the yardstick: the extension steps per second of k_mem_walk on the same index and reads
        ref_rate = json.load(open(mem))["a_reads"]["gpu"]["steps_per_s_kernel"]
        out["a_suffix"]["mem_steps_per_s_kernel"] = ref_rate
        out["a_suffix"]["ratio_to_mem_step_rate"] = round(out["a_suffix"]["gpu"]["steps_per_s_kernel"] / ref_rate, 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
