#!/usr/bin/env python3
"""fetch at scale, on the index of tools/probe_get_pieces.py (K relatives of an L bp genome, both strands: 2 K strings of L symbols) with `ssa -s8`:
(a) ONE region of 1 kbp at the START of string 0 -- wall, engine call, the walk kernel, LF steps -- beside `get 0` on the plain path, `get --pieces 0` and the
    reference's `get 0`, each cut to the region by this probe, the letters compared by md5;
(b) 100 000 random 1 kbp regions (a BED file of string numbers, --row), checked against the strings `get --all` spells;
(c) one whole string as a single region, against `get --pieces 0`.
Walls are medians of --runs runs after a warm-up; kernel times are the HIP events of the command's own `main_fetch` line (RB3_VERBOSE=3).  Every run under a
timeout.  One JSON document, written to --out as well.
    python tools/probe_fetch.py [--K 8] [--L 4000000] [--runs 3] [--regions 100000] [--workdir DIR] [--out profiles/fetch_probe.json]"""
import argparse
import hashlib
import json
import os
import random
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_family  # noqa: E402
from tools.probe_kount import CLI, REF  # noqa: E402

FETCH_LINE = re.compile(rb"(\d+) regions, (\d+) symbols in (\d+) slice\(s\): (\d+) walkers, (\d+) regions measured, (\d+) LF steps, the longest walk of (\d+); "
                        rb"([\d.]+) ms in the engine, table ([\d.]+) ms, plan ([\d.]+) ms, walk ([\d.]+) ms")
GET_LINE = re.compile(rb"(\d+) LF steps; ([\d.]+) ms in the engine")


def run(args, timeout, runs):
    """warm-up + runs: (median / min / max wall, stdout and stderr of the last run); None for a run that failed or ran out of time"""
    env = dict(os.environ, RB3_VERBOSE="3")
    walls, r = [], None
    for i in range(runs + 1):
        t = time.time()
        try:
            r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
        except subprocess.TimeoutExpired:
            return {"timed_out": True}, b"", b""
        if r.returncode != 0:
            return {"rc": r.returncode, "stderr": r.stderr.decode(errors="replace")[-500:]}, b"", b""
        if i > 0:
            walls.append(time.time() - t)
    return {"rc": 0, "wall_s_median": round(statistics.median(walls), 3), "wall_s_min": round(min(walls), 3), "wall_s_max": round(max(walls), 3), "runs": len(walls)}, r.stdout, r.stderr


def letters(stdout):
    """the sequence lines of `get` / `fetch` output"""
    return stdout.split(b"\n")[1::2]


def fetch_stats(err):
    m = FETCH_LINE.search(err)
    if not m:
        return {}
    k = ("regions", "symbols", "slices", "walkers", "measured", "steps", "max_walk_steps")
    out = {a: int(m[i + 1]) for i, a in enumerate(k)}
    out.update({"ms_engine": float(m[8]), "ms_table": float(m[9]), "ms_plan": float(m[10]), "ms_walk": float(m[11])})
    if out["ms_walk"] > 0:
        out["steps_per_s_walk"] = round(out["steps"] / (out["ms_walk"] * 1e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--regions", type=int, default=100000)
    ap.add_argument("--workdir", default="/tmp/rb3_fetch_probe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fetch_probe.json"))
    ap.add_argument("--timeout", type=float, default=200)
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, idx, bed = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd"), os.path.join(a.workdir, "regions.bed")
    t = time.time()
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    subprocess.run([CLI, "ssa", "-s8", "-o", idx + ".ssa", idx], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    out = {"probe": "fetch", "K": a.K, "L": a.L, "n_symbols": 2 * a.K * a.L, "n_strings": 2 * a.K, "ssa_shift": 8, "seconds_build_and_ssa_cli": round(time.time() - t, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def note(tag):
        print(json.dumps({tag: out[tag]}), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:      # (kept up to date: a later run that is cut short leaves the earlier ones)
            f.write(json.dumps(out) + "\n")
    md5 = lambda b: hashlib.md5(b).hexdigest()
    # (a) 1 kbp at the start of string 0
    A = out["a_start_of_string"] = {}
    whole = b""
    A["fetch"], so, se = run([CLI, "fetch", "--row", idx, "0:0-1000"], a.timeout, a.runs)
    A["fetch"].update(fetch_stats(se))
    A["fetch"]["md5"] = md5(letters(so)[0]) if so else None
    for tag, args, runs in (("get_plain", [CLI, "get", idx, "0"], 1), ("get_pieces", [CLI, "get", "--pieces", idx, "0"], a.runs), ("ref_get", [REF, "get", idx, "0"], 1)):
        if args[0] == REF and not os.path.exists(REF):
            continue
        A[tag], go, ge = run(args, a.timeout, runs)
        m = GET_LINE.search(ge)
        if m:
            A[tag].update({"steps": int(m[1]), "ms_engine": float(m[2])})
        if go:
            A[tag]["md5_of_cut"] = md5(letters(go)[0][:1000])
            A[tag]["md5_match"] = A[tag]["md5_of_cut"] == A["fetch"]["md5"]
            if tag == "get_pieces":
                whole = letters(go)[0]
    note("a_start_of_string")
    # (b) random regions of 1 kbp on all strings
    B = out["b_random_regions"] = {}
    g = subprocess.run([CLI, "get", "--all", idx], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=a.timeout)
    strings = letters(g.stdout) if g.returncode == 0 else []
    rng = random.Random(11)
    regs = [(rng.randrange(2 * a.K), rng.randrange(a.L - 1000)) for _ in range(a.regions)]
    with open(bed, "w") as f:
        f.writelines("%d\t%d\t%d\n" % (s, b, b + 1000) for s, b in regs)
    B["fetch"], so, se = run([CLI, "fetch", "--row", "-f", bed, idx], a.timeout, a.runs)
    B["fetch"].update(fetch_stats(se))
    if so and strings:
        B["fetch"]["md5"] = md5(b"".join(letters(so)))
        B["md5_match_get_all"] = B["fetch"]["md5"] == md5(b"".join(strings[s][b:b + 1000] for s, b in regs))
    note("b_random_regions")
    # (c) a whole string as one region
    C = out["c_whole_string"] = {}
    C["fetch"], so, se = run([CLI, "fetch", "--row", idx, "0:0-%d" % a.L], a.timeout, a.runs)
    C["fetch"].update(fetch_stats(se))
    if so:
        C["fetch"]["md5"] = md5(letters(so)[0])
        C["md5_match_get_pieces"] = C["fetch"]["md5"] == md5(whole) if A.get("get_pieces", {}).get("rc") == 0 else None
    C["get_pieces"] = {k: v for k, v in A.get("get_pieces", {}).items() if k.startswith(("wall", "ms_", "steps"))}
    note("c_whole_string")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
