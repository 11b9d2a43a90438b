#!/usr/bin/env python3
"""`overlap --reduce` at scale on reads, beside plain `overlap` from the same build in the same run.
The two workloads of tools/probe_overlap.py: N error-free 150 bp reads of a random genome at 1x and at about 10x, `--pair -l31`.  Per coverage
(a) the two commands in turns -- `overlap`, `overlap --reduce`, `overlap`, ... --, a warm-up of each and then --runs of each: wall (median, min, max), md5 and lines,
    and from the line each prints at -v3 the records before and after, the engine call and its phases (HIP events): COUNT, the rank table, EMIT and, with --reduce,
    REDUCE, COMPACT and the bytes held resident;
(b) in ONE further process on ONE handle: rb3gpu_overlap and rb3gpu_overlap_reduced in turns, the medians of their phases, and what share of the reduced call's GPU
    time REDUCE + COMPACT are beside COUNT + EMIT.
One JSON document, written to --out as well.  Every run under a timeout; the first run that fails, is killed by a signal or times out ends the probe: nothing more
is started on the GPU after it.
    python tools/probe_reduce.py [--reads 1000000] [--coverages 1,10] [--min-len 31] [--runs 3] [--workdir DIR] [--out profiles/reduce_probe.json]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.probe_kount import CLI, run_md5  # noqa: E402
from tools.probe_dedup import must  # noqa: E402
from tools.probe_overlap import MAIN_LINE, generate  # noqa: E402

REDUCE_LINE = re.compile(rb"(\d+) strings: (\d+) overlaps in (\d+) groups of (\d+) strings, (\d+) kept by --reduce, (\d+) groups of (\d+) partners over -c; (\d+) slice\(s\), (\d+) bytes resident; "
                         rb"([\d.]+) ms in the engine: count ([\d.]+), who ([\d.]+), emit ([\d.]+), reduce ([\d.]+), compact ([\d.]+) ms")


def in_turns(cmds, timeout, runs):
    """the commands in turns, a warm-up round first: per command rc, md5, lines, the walls and the last stderr"""
    env = dict(os.environ, RB3_VERBOSE="3")
    out = [{"walls": []} for _ in cmds]
    for i in range(runs + 1):
        for o, cmd in zip(out, cmds):
            wall, rc, md5, lines, err = run_md5(cmd, timeout, env)
            o.update({"rc": rc, "md5": md5, "lines": lines, "timed_out": wall is None, "err": err or b""})
            if wall is None or rc != 0:
                return out
            if i > 0:
                o["walls"].append(wall)
    return out


def summary(o, line, names):
    w = o.pop("walls")
    err = o.pop("err")
    if w:
        o.update({"wall_s_median": round(statistics.median(w), 3), "wall_s_min": round(min(w), 3), "wall_s_max": round(max(w), 3), "runs": len(w)})
    m = line.search(err)
    if m:
        o.update({k: (float(m[i + 1]) if k.startswith("ms_") else int(m[i + 1])) for i, k in enumerate(names)})
    return o


def api(idx, min_len, runs):
    """(b): one handle, the two calls in turns; one JSON line"""
    from ropebwt3_amd import Rb3Gpu
    h = Rb3Gpu(verbose=1)
    out = {}
    try:
        h.from_fmd_file(idx)
        plain, red = [], []
        for _ in range(runs + 1):                            # the first round is the warm-up
            st, sr = {}, {}
            n_all = int(h.overlap(min_len, stats=st).shape[0])
            n_kept = int(h.overlap(min_len, stats=sr, reduce=True).shape[0])
            plain.append(st), red.append(sr)
        med = lambda runs_, k: round(statistics.median(r[k] for r in runs_[1:]), 3)    # noqa: E731
        out["overlap"] = dict({k: med(plain, k) for k in ("ms_total", "ms_count", "ms_who", "ms_emit")}, records=n_all)
        out["reduced"] = dict({k: med(red, k) for k in ("ms_total", "ms_count", "ms_who", "ms_emit", "ms_reduce", "ms_compact")}, records=red[-1]["n_hits"], kept=n_kept,
                              resident_bytes=red[-1]["resident_bytes"])
        r = out["reduced"]
        r["reduce_and_compact_over_count_and_emit"] = round((r["ms_reduce"] + r["ms_compact"]) / (r["ms_count"] + r["ms_emit"]), 3) if r["ms_count"] + r["ms_emit"] > 0 else None
        r["bytes_per_record"] = round(r["resident_bytes"] / r["records"], 2) if r["records"] else None
    finally:
        h.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--coverages", default="1,10")
    ap.add_argument("--min-len", type=int, default=31)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_reduce_probe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_probe.json"))
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--api", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.api:
        return api(a.api, a.min_len, a.runs)
    os.makedirs(a.workdir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = {"probe": "reduce", "reads": a.reads, "read_length": 150, "min_len": a.min_len, "settings": {}}
    for cov in [float(x) for x in a.coverages.split(",")]:
        tag = "%gx" % cov
        txt, idx = os.path.join(a.workdir, "reads_%s.txt" % tag), os.path.join(a.workdir, "reads_%s.fmd" % tag)
        generate(a.reads, cov, txt)
        subprocess.run([CLI, "build", "-L", "-d", "-o", idx, txt], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
        S = {"coverage": cov}
        base = [CLI, "overlap", "--pair", "-l%d" % a.min_len]
        plain, red = in_turns([base + [idx], base + ["--reduce", idx]], a.timeout, a.runs)
        S["cli_overlap"] = must("overlap at %s" % tag, summary(plain, MAIN_LINE, ("strings", "records", "groups", "emitters", "capped_groups", "capped_hits", "steps_count", "steps_emit", "n_early",
                                                                                 "n_slices", "ms_engine", "ms_count", "ms_who", "ms_emit")))
        S["cli_reduce"] = must("overlap --reduce at %s" % tag, summary(red, REDUCE_LINE, ("strings", "records", "groups", "emitters", "kept", "capped_groups", "capped_hits", "n_slices",
                                                                                         "resident_bytes", "ms_engine", "ms_count", "ms_who", "ms_emit", "ms_reduce", "ms_compact")))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--api", idx, "--min-len", str(a.min_len), "--runs", str(a.runs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.timeout)
        must("the two calls on one handle at %s" % tag, {"rc": r.returncode})
        S["same_handle"] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        out["settings"][tag] = S
        print(json.dumps({tag: S}), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:      # (kept up to date: a later run that is cut short leaves the earlier ones)
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
