#!/usr/bin/env python3
"""`dedup` at scale on reads with a KNOWN share of copies and substrings.
N error-free 150 bp reads are drawn from a random genome at 1x coverage (tools/gen_reads.py's sampling without its errors; seed 4); a share --copies of them
is written a second time, half of those as reverse complements, and a share --subs of them contributes a substring of 60 .. 120 bp.  Reported:
(a) `dedup --pair`: wall (median of --runs after a warm-up), the engine call, the walk (HIP events), steps, steps per second, the share of walks that ended
    early, duplicates and contained found beside the numbers planted (reads that overlap by chance make the found numbers no smaller than the planted ones);
    the same with RB3GPU_DEDUP_EARLY=0;
(b) the pipeline `dedup --pair X | remove --pair -d -f - X` beside `build -d -L` of the surviving reads with this CLI and, where it is there, the reference; md5s.
One JSON document, written to --out as well.  Every run under a timeout; the first run that fails, is killed by a signal or times out ends the probe:
nothing more is started on the GPU after it.
    python tools/probe_dedup.py [--reads 1000000] [--copies 0.05] [--subs 0.05] [--runs 3] [--workdir DIR] [--out profiles/dedup_probe.json]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.probe_kount import run_md5, CLI, REF  # noqa: E402
from tools.probe_remove import timed, rate  # noqa: E402

MAIN_LINE = re.compile(rb"(\d+) strings: (\d+) duplicates, (\d+) contained, (\d+) classes of copies; (\d+) steps in (\d+) slice\(s\), (\d+) walks ended early; ([\d.]+) ms in the engine, walk ([\d.]+) ms")
ALPH = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def generate(N, copies, subs, fn, seed=4):
    """the reads, one per line; returns (lines written, copies planted, substrings planted)"""
    rng = np.random.default_rng(seed)
    G = ALPH[rng.integers(0, 4, size=max(1000, N * 150))]            # 1x: reads overlap, none lies inside another by chance (all are 150 bp)
    st = rng.integers(0, len(G) - 150, size=N)
    n_copy = n_sub = 0
    with open(fn, "wb") as f:
        for i in range(N):
            r = G[st[i]:st[i] + 150].tobytes()
            f.write(r + b"\n")
            u = rng.random()
            if u < copies:
                f.write((r if n_copy % 2 == 0 else r.translate(COMP)[::-1]) + b"\n")
                n_copy += 1
            elif u < copies + subs:
                ln = int(rng.integers(60, 121))
                a = int(rng.integers(0, 150 - ln + 1))
                f.write(r[a:a + ln] + b"\n")
                n_sub += 1
    return N + n_copy + n_sub, n_copy, n_sub


def dedup_run(args, timeout, runs, env=None):
    out, err = timed([CLI, "dedup"] + args, timeout, runs, env)
    m = MAIN_LINE.search(err)
    if m:
        out.update({"strings": int(m[1]), "n_dup": int(m[2]), "n_contained": int(m[3]), "n_classes": int(m[4]), "steps": int(m[5]), "n_slices": int(m[6]), "n_early": int(m[7]),
                    "ms_engine": float(m[8]), "ms_walk": float(m[9])})
        out["steps_per_s"], out["early_share"] = rate(int(m[5]), float(m[9])), round(int(m[7]) / max(int(m[1]), 1), 4)
    return out


def must(tag, run):
    """end the probe where a run did not end well: nothing more is started on the GPU after a failure, a signal or a timeout"""
    if run.get("timed_out") or run.get("rc") != 0:
        print(json.dumps({"stopped_at": tag, "rc": run.get("rc"), "timed_out": run.get("timed_out")}), flush=True)
        sys.exit(1)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--copies", type=float, default=0.05)
    ap.add_argument("--subs", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_dedup_probe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_probe.json"))
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--ref-timeout", type=float, default=300)
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    txt, idx, rest, drop = (os.path.join(a.workdir, x) for x in ("reads.txt", "reads.fmd", "rest.txt", "drop.txt"))
    n_lines, n_copy, n_sub = generate(a.reads, a.copies, a.subs, txt)
    subprocess.run([CLI, "build", "-L", "-d", "-o", idx, txt], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    out = {"probe": "dedup", "reads": a.reads, "sequences": n_lines, "planted_copies": n_copy, "planted_substrings": n_sub, "n_symbols": None}
    out["n_symbols"] = 2 * (sum(len(x) for x in open(txt, "rb")))

    def note(tag):
        print(json.dumps({tag: out[tag]}), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:      # (kept up to date: a later run that is cut short leaves the earlier ones)
            f.write(json.dumps(out) + "\n")
    # (a) the command, with and without the early exit
    A = {"early": must("dedup", dedup_run(["--pair", idx], a.timeout, a.runs))}
    A["no_early"] = must("dedup without the early exit", dedup_run(["--pair", idx], a.timeout, 1, {"RB3GPU_DEDUP_EARLY": "0"}))
    A["same_list"] = A["early"]["md5"] == A["no_early"]["md5"] if A["early"]["md5"] else None
    out["a_dedup"] = A
    note("a_dedup")
    # (b) the pipeline through remove beside build -d of the survivors
    r = subprocess.run([CLI, "dedup", "--pair", idx], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=a.timeout, check=True)
    open(drop, "wb").write(r.stdout)
    gone = {int(x) for x in r.stdout.split()}
    with open(txt, "rb") as fi, open(rest, "wb") as f:
        for i, line in enumerate(fi):
            if i not in gone:
                f.write(line)
    B = {"dropped": len(gone)}
    B["remove"] = must("remove", timed([CLI, "remove", "--pair", "-d", "-f", drop, idx], a.timeout, 1)[0])
    B["cli_build"] = must("build of the survivors", timed([CLI, "build", "-L", "-d", rest], a.timeout, 1)[0])
    B["cli_build"]["md5_match"] = B["cli_build"]["md5"] == B["remove"]["md5"] if B["remove"]["md5"] else None
    if os.path.exists(REF):
        nt = min(16, os.cpu_count() or 8)
        wall, rc, md5, _, _ = run_md5([REF, "build", "-L", "-d", "-t%d" % nt, rest], a.ref_timeout)
        B["ref_build"] = {"wall_s": round(wall, 3) if wall else None, "rc": rc, "md5": md5, "timed_out": wall is None, "threads": nt, "md5_match": md5 == B["remove"]["md5"] if md5 else None}
    out["b_pipeline"] = B
    note("b_pipeline")
    out["drop_md5"] = hashlib.md5(r.stdout).hexdigest()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
