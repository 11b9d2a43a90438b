#!/usr/bin/env python3
"""`overlap` at scale on reads: where most reads overlap a few others, and where they hardly do.
N error-free 150 bp reads are drawn from a random genome (the sampling of tools/probe_dedup.py, seed 4, without its planted copies) at every coverage of
--coverages: 1x, the setting of probe_dedup.py, and about 10x, where most reads overlap.  Per coverage and per minimum length of --min-lens (31 and 75):
(a) `overlap --pair -l L`: wall (median of --runs after a warm-up), md5 and lines, and from the command's line at -v3 the engine call, the three phases (HIP events),
    the steps of the COUNT and of the EMIT walk with their steps per second, the share of walks that ended early, records, groups, emitters;
(b) in ONE further process on ONE handle: rb3gpu_overlap at every minimum length (the counting walk alone is what is compared) and rb3gpu_dedup, whose walk goes
    down the same chains with five rank loads a step where k_ovl_walk has three -- the yardstick: steps per second of both, and their ratio.
One JSON document, written to --out as well.  Every run under a timeout; the first run that fails, is killed by a signal or times out ends the probe:
nothing more is started on the GPU after it.
    python tools/probe_overlap.py [--reads 1000000] [--coverages 1,10] [--min-lens 31,75] [--runs 3] [--workdir DIR] [--out profiles/overlap_probe.json]"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.probe_kount import CLI  # noqa: E402
from tools.probe_remove import timed, rate  # noqa: E402
from tools.probe_dedup import must  # noqa: E402

MAIN_LINE = re.compile(rb"(\d+) strings: (\d+) overlaps in (\d+) groups of (\d+) strings, (\d+) groups of (\d+) partners over -c; (\d+) \+ (\d+) steps, (\d+) walks ended early, (\d+) slice\(s\); "
                       rb"([\d.]+) ms in the engine: count ([\d.]+), who ([\d.]+), emit ([\d.]+) ms")
ALPH = np.frombuffer(b"ACGT", dtype=np.uint8)


def generate(N, coverage, fn, seed=4):
    """N reads of 150 bp, one per line, from a genome of N * 150 / coverage bp"""
    rng = np.random.default_rng(seed)
    G = ALPH[rng.integers(0, 4, size=max(1000, int(N * 150 / coverage)))]
    st = rng.integers(0, len(G) - 150, size=N)
    with open(fn, "wb") as f:
        for i in range(N):
            f.write(G[st[i]:st[i] + 150].tobytes() + b"\n")


def overlap_run(args, timeout, runs):
    out, err = timed([CLI, "overlap"] + args, timeout, runs)
    m = MAIN_LINE.search(err)
    if m:
        v = [int(m[i]) for i in range(1, 11)] + [float(m[i]) for i in range(11, 15)]
        out.update(dict(zip(("strings", "records", "groups", "emitters", "capped_groups", "capped_hits", "steps_count", "steps_emit", "n_early", "n_slices", "ms_engine", "ms_count",
                             "ms_who", "ms_emit"), v)))
        out["count_steps_per_s"], out["emit_steps_per_s"], out["early_share"] = rate(v[6], v[11]), rate(v[7], v[13]), round(v[8] / max(v[0], 1), 4)
    return out


def api(idx, min_lens, runs):
    """(b): one handle, rb3gpu_overlap and rb3gpu_dedup side by side; one JSON line"""
    import statistics
    from ropebwt3_amd import Rb3Gpu
    h = Rb3Gpu(verbose=1)
    out = {}
    try:
        h.from_fmd_file(idx)
        for L in min_lens:
            ms, st = [], {}
            for _ in range(runs + 1):                        # the first run is the warm-up
                rec = h.overlap(L, stats=st)
                ms.append(st["ms_count"])
            m = statistics.median(ms[1:])
            out["overlap_l%d" % L] = {"ms_count": round(m, 3), "steps": st["n_steps_count"], "steps_per_s": rate(st["n_steps_count"], m), "records": int(rec.shape[0]), "ms_who": round(st["ms_who"], 3),
                                      "ms_emit": round(st["ms_emit"], 3), "emit_steps": st["n_steps_emit"]}
            del rec
        ms, st = [], {}
        for _ in range(runs + 1):
            h.dedup(pair=True, stats=st)
            ms.append(st["ms_walk"])
        m = statistics.median(ms[1:])
        out["dedup"] = {"ms_walk": round(m, 3), "steps": st["n_steps"], "steps_per_s": rate(st["n_steps"], m)}
        for L in min_lens:
            o = out["overlap_l%d" % L]
            o["rate_over_dedup"] = round(o["steps_per_s"] / out["dedup"]["steps_per_s"], 3) if o["steps_per_s"] and out["dedup"]["steps_per_s"] else None
    finally:
        h.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--coverages", default="1,10")
    ap.add_argument("--min-lens", default="31,75")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_overlap_probe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_probe.json"))
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--api", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    min_lens = [int(x) for x in a.min_lens.split(",")]
    if a.api:
        return api(a.api, min_lens, a.runs)
    os.makedirs(a.workdir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = {"probe": "overlap", "reads": a.reads, "read_length": 150, "settings": {}}
    for cov in [float(x) for x in a.coverages.split(",")]:
        tag = "%gx" % cov
        txt, idx = os.path.join(a.workdir, "reads_%s.txt" % tag), os.path.join(a.workdir, "reads_%s.fmd" % tag)
        generate(a.reads, cov, txt)
        subprocess.run([CLI, "build", "-L", "-d", "-o", idx, txt], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
        S = {"coverage": cov, "n_symbols": 2 * sum(len(x) for x in open(txt, "rb"))}
        for L in min_lens:
            S["cli_l%d" % L] = must("overlap -l%d at %s" % (L, tag), overlap_run(["--pair", "-l%d" % L, idx], a.timeout, a.runs))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--api", idx, "--min-lens", a.min_lens, "--runs", str(a.runs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.timeout)
        must("the API beside dedup at %s" % tag, {"rc": r.returncode})
        S["same_handle"] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        out["settings"][tag] = S
        print(json.dumps({tag: S}), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:      # (kept up to date: a later run that is cut short leaves the earlier ones)
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
