#!/usr/bin/env python3
"""`unitig` at scale on reads, beside what a user had to run before it existed: `overlap --pair --reduce` followed by `get --all`, from the same build in the same run.
The reads of tools/probe_reduce.py: N error-free 150 bp reads of a random genome at 1x and at about 10x, after `dedup --pair | remove --pair`, `--pair -l31`.  Per coverage
(a) the three commands in turns -- `unitig`, `overlap --reduce`, `get --all`, `unitig`, ... --, a warm-up of each and then --runs of each: wall (median, min, max), md5
    and lines; from the line `unitig` prints at -v3 the counters, the engine call and its phases (HIP events): the reduce stages, graph, rank, emit;
(b) in ONE further process on ONE handle: rb3gpu_unitigs --runs times after a warm-up, the medians of its phases, the emit step rate beside that of k_get_walk<true>
    over all the strings of the same index (symbols per second of the emitting launches), n_rounds, the unitig N50 and the resident bytes.
One JSON document, written to --out as well.  Every run under a timeout; the first run that fails, is killed by a signal or times out ends the probe: nothing more
is started on the GPU after it.
    python tools/probe_unitig.py [--reads 1000000] [--coverages 1,10] [--min-len 31] [--runs 3] [--workdir DIR] [--out profiles/unitig_probe.json]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.probe_kount import CLI  # noqa: E402
from tools.probe_dedup import must  # noqa: E402
from tools.probe_overlap import generate  # noqa: E402
from tools.probe_reduce import REDUCE_LINE, in_turns, summary  # noqa: E402

UNITIG_LINE = re.compile(rb"(\d+) strings: (\d+) kept overlaps, (\d+) simple; (\d+) unitigs of (\d+) members and (\d+) symbols, (\d+) circular, longest (\d+) members, (\d+) links; "
                         rb"(\d+) rounds, (\d+) steps, (\d+) slice\(s\), (\d+) bytes resident; ([\d.]+) ms in the engine: reduce ([\d.]+), graph ([\d.]+), rank ([\d.]+), emit ([\d.]+) ms")
UNITIG_NAMES = ("strings", "kept", "simple", "unitigs", "members", "symbols", "cycles", "max_members", "links", "rounds", "steps_emit", "n_slices", "resident_bytes",
                "ms_engine", "ms_reduce", "ms_graph", "ms_rank", "ms_emit")


def n50(lens):
    lens = sorted((int(x) for x in lens), reverse=True)
    half, tot = sum(lens) / 2, 0
    for x in lens:
        tot += x
        if tot >= half:
            return x
    return 0


def api(idx, min_len, runs):
    """(b): one handle; one JSON line"""
    from ropebwt3_amd import Rb3Gpu
    h = Rb3Gpu(verbose=1)
    out = {}
    try:
        h.from_fmd_file(idx)
        got, utg = [], None
        for _ in range(runs + 1):                            # the first call is the warm-up
            st = {}
            utg = h.unitigs(min_len, pair=True, stats=st)[0]
            got.append(st)
        med = lambda k: round(statistics.median(r[k] for r in got[1:]), 3)    # noqa: E731
        last = got[-1]
        out["unitigs"] = dict({k: med(k) for k in ("ms_total", "ms_reduce", "ms_graph", "ms_rank", "ms_emit")},
                              **{k: last[k] for k in ("n_strings", "n_kept", "n_simple", "n_unitigs", "n_members", "n_symbols", "n_steps_emit", "n_cycles", "n_links", "n_rounds",
                                                      "max_members", "n_slices", "resident_bytes")})
        u = out["unitigs"]
        u["n50"] = n50(utg["len"])
        u["emit_steps_per_s"] = round(u["n_steps_emit"] / (u["ms_emit"] * 1e-3)) if u["ms_emit"] > 0 else None
        u["bytes_per_string"] = round(u["resident_bytes"] / u["n_strings"], 1)
        del utg
        m = int(h.get_acc()[1])
        gs = []
        for _ in range(runs + 1):
            st = {}
            h.retrieve(range(m), stats=st)
            gs.append(st)
        ms = statistics.median(r["ms_emit"] for r in gs[1:])
        out["get"] = {"n_rows": m, "n_symbols": gs[-1]["n_symbols"], "ms_emit": round(ms, 3), "emit_symbols_per_s": round(gs[-1]["n_symbols"] / (ms * 1e-3)) if ms > 0 else None}
    finally:
        h.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--coverages", default="1,10")
    ap.add_argument("--min-len", type=int, default=31)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_unitig_probe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitig_probe.json"))
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--api", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.api:
        return api(a.api, a.min_len, a.runs)
    os.makedirs(a.workdir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = {"probe": "unitig", "reads": a.reads, "read_length": 150, "min_len": a.min_len, "settings": {}}
    for cov in [float(x) for x in a.coverages.split(",")]:
        tag = "%gx" % cov
        txt, full, idx, drop = (os.path.join(a.workdir, "reads_%s.%s" % (tag, e)) for e in ("txt", "full.fmd", "fmd", "drop"))
        generate(a.reads, cov, txt)
        subprocess.run([CLI, "build", "-L", "-d", "-o", full, txt], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
        with open(drop, "wb") as f:                          # dedup --pair | remove --pair: what the pipeline runs in front of unitig
            must("dedup at %s" % tag, {"rc": subprocess.run([CLI, "dedup", "--pair", full], stdout=f, stderr=subprocess.DEVNULL, timeout=a.timeout).returncode})
        must("remove at %s" % tag, {"rc": subprocess.run([CLI, "remove", "--pair", "-d", "-o", idx, "-f", drop, full], stderr=subprocess.DEVNULL, timeout=a.timeout).returncode})
        S = {"coverage": cov, "dropped": sum(1 for _ in open(drop, "rb"))}
        utg, red, get = in_turns([[CLI, "unitig", "--pair", "-l%d" % a.min_len, idx], [CLI, "overlap", "--pair", "--reduce", "-l%d" % a.min_len, idx], [CLI, "get", "--all", idx]],
                                 a.timeout, a.runs)
        S["cli_unitig"] = must("unitig at %s" % tag, summary(utg, UNITIG_LINE, UNITIG_NAMES))
        S["cli_reduce"] = must("overlap --reduce at %s" % tag, summary(red, REDUCE_LINE, ("strings", "records", "groups", "emitters", "kept", "capped_groups", "capped_hits", "n_slices",
                                                                                         "resident_bytes", "ms_engine", "ms_count", "ms_who", "ms_emit", "ms_reduce", "ms_compact")))
        S["cli_get_all"] = must("get --all at %s" % tag, summary(get, UNITIG_LINE, ()))
        if "wall_s_median" in S["cli_reduce"] and "wall_s_median" in S["cli_get_all"]:
            S["wall_s_reduce_then_get"] = round(S["cli_reduce"]["wall_s_median"] + S["cli_get_all"]["wall_s_median"], 3)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--api", idx, "--min-len", str(a.min_len), "--runs", str(a.runs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.timeout)
        must("the calls on one handle at %s" % tag, {"rc": r.returncode})
        S["same_handle"] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        out["settings"][tag] = S
        print(json.dumps({tag: S}), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:      # (kept up to date: a later run that is cut short leaves the earlier ones)
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
