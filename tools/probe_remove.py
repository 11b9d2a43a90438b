#!/usr/bin/env python3
"""`remove` at scale against rebuilding what stays.
(a) the seeded index of tools/probe_mem.py (K relatives of an L bp genome, both strands: 2 K strings of L symbols): one relative (2 strings) taken out with
    --pieces and on the plain path -- wall, the engine call, marking, rebuild, marking steps per second --, next to `build -d` of the K - 1 relatives that stay
    with this repository's own CLI (the build path is the parent's: `remove` adds a command, it changes none) and with the reference binary; md5s compared;
(b) an index of N simulated reads: every tenth read taken out on the plain path, against the same two rebuilds;
(c) the marking walk beside the COUNT walk it restates, from the same runs: `remove --pieces` reports its counting walk over all pieces (k_piece_walk<false>) and
    its marking walk (k_mark_pieces); `get` of the same two strings on the plain path reports the counting walk of k_get_walk for k_mark_walk.
One JSON document, written to --out as well.  Every run under a timeout.
    python tools/probe_remove.py [--K 8] [--L 4000000] [--reads 100000] [--runs 2] [--workdir DIR] [--out profiles/remove_probe.json]"""
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
from tools import gen_family, gen_reads  # noqa: E402
from tools.probe_kount import run_md5, CLI, REF  # noqa: E402

MAIN_LINE = re.compile(rb"removed (\d+) strings, (\d+) rows .*?: (\d+) LF steps, (\d+) pieces, the longest of (\d+) steps; ([\d.]+) ms in the engine, marking ([\d.]+) ms, rebuild ([\d.]+) ms")
PIECES_LINE = re.compile(rb"in pieces: counting walk ([\d.]+) ms \((\d+) steps\), join ([\d.]+) ms, marking walk ([\d.]+) ms \((\d+) steps\)")
PLAIN_LINE = re.compile(rb"strings: marking walk ([\d.]+) ms \((\d+) steps\)")
GET_LINE = re.compile(rb"(\d+) LF steps; ([\d.]+) ms in the engine, counting walk ([\d.]+) ms, writing walk ([\d.]+) ms")


def rate(steps, ms):
    return round(steps / (ms * 1e-3)) if ms > 0 else None


def timed(cmd, timeout, runs, env=None):
    env = dict(os.environ, RB3_VERBOSE="3", **(env or {}))
    walls, last = [], None
    for i in range(runs + 1):   # the first run is the warm-up
        last = run_md5(cmd, timeout, env)
        if last[0] is None or last[1] != 0:
            break
        if i > 0:
            walls.append(last[0])
    wall, rc, md5, _, err = last
    out = {"rc": rc, "md5": md5, "timed_out": wall is None}
    if walls:
        out.update({"wall_s_median": round(statistics.median(walls), 3), "wall_s_min": round(min(walls), 3), "wall_s_max": round(max(walls), 3), "runs": len(walls)})
    return out, err or b""


def remove_run(args, timeout, runs):
    out, err = timed([CLI, "remove", "-d"] + args, timeout, runs)
    m = MAIN_LINE.search(err)
    if m:
        out.update({"strings": int(m[1]), "rows": int(m[2]), "steps": int(m[3]), "n_pieces": int(m[4]), "max_piece_steps": int(m[5]), "ms_engine": float(m[6]), "ms_mark": float(m[7]), "ms_build": float(m[8])})
    m = PIECES_LINE.search(err)
    if m:
        out.update({"ms_count_walk": float(m[1]), "count_steps": int(m[2]), "ms_join": float(m[3]), "ms_mark_walk": float(m[4]), "mark_steps": int(m[5])})
        out["count_steps_per_s"], out["mark_steps_per_s"] = rate(int(m[2]), float(m[1])), rate(int(m[5]), float(m[4]))
    m = PLAIN_LINE.search(err)
    if m:
        out.update({"ms_mark_walk": float(m[1]), "mark_steps": int(m[2]), "mark_steps_per_s": rate(int(m[2]), float(m[1]))})
    return out


def rebuilds(rest_fa, flags, want_md5, timeout, ref_timeout, runs):
    """`build -d` of what stays: this CLI (the parent's build path) and the reference"""
    out = {}
    r, _ = timed([CLI, "build", "-d"] + flags + [rest_fa], timeout, runs)
    r["md5_match"] = r["md5"] == want_md5 if r["md5"] else None
    out["cli_build"] = r
    if os.path.exists(REF):
        nt = min(16, os.cpu_count() or 8)
        wall, rc, md5, _, _ = run_md5([REF, "build", "-d", "-t%d" % nt] + flags + [rest_fa], ref_timeout)
        out["ref_build"] = {"wall_s": round(wall, 3) if wall else None, "rc": rc, "md5": md5, "timed_out": wall is None, "threads": nt, "md5_match": md5 == want_md5 if md5 else None}
    return out


def records(fn):
    recs, name, seq = [], None, []
    for line in open(fn):
        if line.startswith(">"):
            if name is not None:
                recs.append((name, "".join(seq)))
            name, seq = line.strip(), []
        else:
            seq.append(line.strip())
    if name is not None:
        recs.append((name, "".join(seq)))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--workdir", default="/tmp/rb3_remove_probe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove_probe.json"))
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--ref-timeout", type=float, default=300)
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = {"probe": "remove", "K": a.K, "L": a.L, "reads": a.reads}

    def note(tag):
        print(json.dumps({tag: out[tag]}), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:      # (kept up to date: a later run that is cut short leaves the earlier ones)
            f.write(json.dumps(out) + "\n")
    # (a) one relative out of K
    fa, idx, rest = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd"), os.path.join(a.workdir, "rel_rest.fa")
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    gone = a.K // 2
    with open(rest, "w") as f:
        for i, (name, seq) in enumerate(records(fa)):
            if i != gone:
                f.write("%s\n%s\n" % (name, seq))
    A = {"n_symbols": 2 * a.K * a.L, "sequence": gone}
    A["pieces"] = remove_run(["--pieces", "--pair", idx, str(gone)], a.timeout, a.runs)
    A["plain"] = remove_run(["--pair", idx, str(gone)], a.timeout, 1)
    A["md5_match"] = A["plain"]["md5"] == A["pieces"]["md5"] if A["plain"]["md5"] else None
    A.update(rebuilds(rest, [], A["pieces"]["md5"], a.timeout, a.ref_timeout, a.runs))
    out["a_one_relative"] = A
    note("a_one_relative")
    # (c) the marking walks beside the counting walks they restate
    g, err = timed([CLI, "get", idx, str(2 * gone), str(2 * gone + 1)], a.timeout, 0)
    C = {"pieces_count_steps_per_s": A["pieces"].get("count_steps_per_s"), "pieces_mark_steps_per_s": A["pieces"].get("mark_steps_per_s"), "plain_mark_steps_per_s": A["plain"].get("mark_steps_per_s")}
    m = GET_LINE.search(err)
    if m:                                # (the steps of `get` are those of its two walks: half of them are the counting walk's)
        C["plain_count_steps_per_s"] = rate(int(m[1]) // 2, float(m[3]))
    for k in ("pieces", "plain"):
        c, mk = C.get(k + "_count_steps_per_s"), C.get(k + "_mark_steps_per_s")
        if c and mk:
            C[k + "_mark_over_count"] = round(mk / c, 3)
    C["note"] = "the marking walk of the pieces runs only the pieces of the strings asked for: fewer walkers in flight than the counting walk over all pieces"
    out["c_mark_beside_count"] = C
    note("c_mark_beside_count")
    # (b) a tenth of the reads
    rfa, ridx, rrest, rrows = os.path.join(a.workdir, "reads.txt"), os.path.join(a.workdir, "reads.fmd"), os.path.join(a.workdir, "reads_rest.txt"), os.path.join(a.workdir, "reads_rows.txt")
    gen_reads.generate(a.reads, rfa)     # (one read per line: build -L)
    subprocess.run([CLI, "build", "-L", "-d", "-o", ridx, rfa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    n_reads = 0
    with open(rfa) as fi, open(rrest, "w") as f, open(rrows, "w") as fr:
        for i, line in enumerate(fi):
            n_reads += 1
            if i % 10 == 0:
                fr.write("%d\n" % i)
            else:
                f.write(line)
    Bp = {"n_reads": n_reads, "removed": (n_reads + 9) // 10}
    Bp["plain"] = remove_run(["--pair", "-f", rrows, ridx], a.timeout, a.runs)
    Bp.update(rebuilds(rrest, ["-L"], Bp["plain"]["md5"], a.timeout, a.ref_timeout, a.runs))
    out["b_tenth_of_reads"] = Bp
    note("b_tenth_of_reads")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
