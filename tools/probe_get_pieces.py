#!/usr/bin/env python3
"""get in pieces at scale, on the seeded index of tools/probe_mem.py (K relatives of an L bp genome, both strands: 2 K strings of L symbols):
(a) `get 0` -- ONE string of L symbols -- on the plain path, `get --pieces 0`, and the reference's `get 0`;
(b) `get --all` against the reference's `get 0 1 .. 2K-1`;
(c) `get --all` with RB3GPU_GET_PIECE swept over --sweep: the four phases, the number of pieces, the longest piece, steps per second.
The yardsticks are the plain path (which this option leaves untouched) and the reference binary on the same machine.  Every run under a timeout.
One JSON document, written to --out as well: wall times (warm-up + --runs runs: median, min, max), md5 of the outputs and whether they agree.
    python tools/probe_get_pieces.py [--K 8] [--L 4000000] [--runs 2] [--sweep 4,5,..,12] [--workdir DIR] [--out profiles/get_pieces_probe.json]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_family  # noqa: E402
from tools.probe_kount import run_md5, CLI, REF  # noqa: E402

GET_LINE = re.compile(rb"(\d+) rows, (\d+) symbols in (\d+) slice\(s\): (\d+) LF steps; ([\d.]+) ms in the engine, counting walk ([\d.]+) ms, writing walk ([\d.]+) ms")
PIECES_LINE = re.compile(rb"(\d+) rows, (\d+) symbols in (\d+) slice\(s\): (\d+) pieces, the longest of (\d+) steps, (\d+) LF steps; ([\d.]+) ms in the engine, "
                         rb"pieces ([\d.]+) ms, join ([\d.]+) ms, sort ([\d.]+) ms, writing walk ([\d.]+) ms")


def cli_run(args, timeout, runs, env=None):
    env = dict(os.environ, RB3_VERBOSE="3", **(env or {}))
    walls, last = [], None
    for i in range(runs + 1):   # the first run is the warm-up
        last = run_md5([CLI, "get"] + args, timeout, env)
        if last[0] is None or last[1] != 0:
            break
        if i > 0:
            walls.append(last[0])
    wall, rc, md5, lines, err = last
    out = {"rc": rc, "md5": md5, "lines": lines, "timed_out": wall is None}
    if walls:
        out.update({"wall_s_median": round(statistics.median(walls), 3), "wall_s_min": round(min(walls), 3), "wall_s_max": round(max(walls), 3), "runs": len(walls)})
    m = PIECES_LINE.search(err or b"")
    if m:
        steps, ph = int(m[6]), [float(m[i]) for i in (8, 9, 10, 11)]
        out.update({"rows": int(m[1]), "symbols": int(m[2]), "slices": int(m[3]), "n_pieces": int(m[4]), "max_piece_steps": int(m[5]), "steps": steps, "ms_engine": float(m[7]),
                    "ms_pieces": ph[0], "ms_join": ph[1], "ms_sort": ph[2], "ms_emit": ph[3],
                    "steps_per_s_kernel": round(steps / ((ph[0] + ph[3]) * 1e-3)) if ph[0] + ph[3] > 0 else None})
    else:
        m = GET_LINE.search(err or b"")
        if m:
            steps, ms_count, ms_emit = int(m[4]), float(m[6]), float(m[7])
            out.update({"rows": int(m[1]), "symbols": int(m[2]), "slices": int(m[3]), "steps": steps, "ms_engine": float(m[5]), "ms_count": ms_count, "ms_emit": ms_emit,
                        "steps_per_s_kernel": round(steps / ((ms_count + ms_emit) * 1e-3)) if ms_count + ms_emit > 0 else None})
    return out


def ref_run(args, timeout, g):
    wall, rc, md5, lines, _ = run_md5([REF, "get"] + args, timeout)
    r = {"wall_s": round(wall, 3) if wall else None, "rc": rc, "md5": md5, "timed_out": wall is None, "threads": 1}
    r["md5_match"] = r["md5"] == g["md5"] if r["md5"] else None
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--sweep", default="4,5,6,7,8,9,10,11,12")
    ap.add_argument("--workdir", default="/tmp/rb3_get_pieces_probe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "get_pieces_probe.json"))
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--ref-timeout", type=float, default=300)
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, idx = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd")
    t = time.time()
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    out = {"probe": "get_pieces", "K": a.K, "L": a.L, "n_symbols": 2 * a.K * a.L, "n_strings": 2 * a.K, "seconds_build_cli": round(time.time() - t, 2)}
    rows = [str(i) for i in range(2 * a.K)]

    def note(tag):
        print(json.dumps({tag: out[tag]}), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:      # (kept up to date: a later run that is cut short leaves the earlier ones)
            f.write(json.dumps(out) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    # (a) one string
    out["a_one_string"] = {"plain": cli_run([idx, "0"], a.timeout, 1), "pieces": cli_run(["--pieces", idx, "0"], a.timeout, a.runs)}
    A = out["a_one_string"]
    A["md5_match"] = A["plain"]["md5"] == A["pieces"]["md5"] if A["plain"]["md5"] else None
    if os.path.exists(REF):
        A["ref_t1"] = ref_run([idx, "0"], a.ref_timeout, A["pieces"])
    for k in ("plain", "ref_t1"):
        w = A.get(k, {}).get("wall_s_median") or A.get(k, {}).get("wall_s")
        if w and A["pieces"].get("wall_s_median"):
            A["pieces_speedup_over_" + k] = round(w / A["pieces"]["wall_s_median"], 2)
    note("a_one_string")
    # (b) all the strings
    out["b_all"] = {"pieces": cli_run(["--all", idx], a.timeout, a.runs)}
    B = out["b_all"]
    if os.path.exists(REF):
        B["ref_t1"] = ref_run([idx] + rows, a.ref_timeout, B["pieces"])
        if B["ref_t1"]["wall_s"] and B["pieces"].get("wall_s_median"):
            B["pieces_speedup_over_ref_t1"] = round(B["ref_t1"]["wall_s"] / B["pieces"]["wall_s_median"], 2)
    note("b_all")
    # (c) the spacing
    out["c_sweep"] = {}
    for S in [int(x) for x in a.sweep.split(",") if x]:
        out["c_sweep"][str(S)] = cli_run(["--all", idx], a.timeout, 1, {"RB3GPU_GET_PIECE": str(S)})
        out["c_sweep"][str(S)]["md5_match"] = out["c_sweep"][str(S)]["md5"] == B["pieces"]["md5"]
    note("c_sweep")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
