#!/usr/bin/env python3
"""kount at scale: builds a seeded index with the CLI (K relatives of an L bp genome, tools/gen_family.py; both strands: 2 K L
symbols), then runs `ropebwt3-amd kount -k51 -m2` and the reference's `kount` with the same arguments, each under a timeout, and
prints one JSON line: both wall times, whether the md5 of their outputs match, nodes expanded, GPU ms, expansions per second, output
lines and the host time spent formatting them (the CLI's -v3 line).
    python tools/probe_kount.py [--K 8] [--L 4000000] [--k 51] [--m 2] [--workdir DIR] [--ref-timeout 400]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_family  # noqa: E402

CLI = os.path.join(ROOT, "ropebwt3_amd", "ropebwt3-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "ropebwt3")


def run_md5(cmd, timeout, env=None):
    """wall time, exit status, md5 and lines of stdout (streamed), stderr; (None, ...) on a timeout"""
    t = time.time()
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    md5, lines = hashlib.md5(), 0
    err = []
    th = threading.Thread(target=lambda: err.append(p.stderr.read()))
    th.start()
    try:
        while True:
            if time.time() - t > timeout:
                raise subprocess.TimeoutExpired(cmd, timeout)
            b = p.stdout.read(1 << 22)
            if not b:
                break
            md5.update(b)
            lines += b.count(b"\n")
        p.wait(timeout=max(1, timeout - (time.time() - t)))
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
        th.join()
        return None, None, None, None, b"".join(err)
    th.join()
    return time.time() - t, p.returncode, md5.hexdigest(), lines, b"".join(err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--k", type=int, default=51)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--workdir", default="/tmp/rb3_kount_probe")
    ap.add_argument("--timeout", type=float, default=300)
    ap.add_argument("--ref-timeout", type=float, default=400)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    fa, idx = os.path.join(a.workdir, "rel.fa"), os.path.join(a.workdir, "rel.fmd")
    t = time.time()
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", idx, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    t_build = time.time() - t
    args = ["kount", "-k%d" % a.k, "-m%d" % a.m, idx]
    env = dict(os.environ, RB3_VERBOSE="3")
    wall, rc, md5, lines, err = run_md5([CLI] + args, a.timeout, env)
    out = {"probe": "kount", "K": a.K, "L": a.L, "k": a.k, "m": a.m, "n_symbols": 2 * a.K * a.L, "seconds_build_cli": round(t_build, 2),
           "gpu_wall_s": round(wall, 3) if wall else None, "gpu_rc": rc, "lines": lines, "gpu_md5": md5}
    mm = re.search(rb"(\d+) k-mers; (\d+) nodes expanded in (\d+) slice\(s\): ([\d.]+) ms in the engine, of which ([\d.]+) ms formatting lines; "
                   rb"expansion kernel ([\d.]+) ms", err or b"")
    if mm:
        n_out, nodes, slices, ms_total, ms_fmt, ms_exp = int(mm[1]), int(mm[2]), int(mm[3]), float(mm[4]), float(mm[5]), float(mm[6])
        out.update({"n_out": n_out, "nodes": nodes, "slices": slices, "ms_engine": ms_total, "ms_format": ms_fmt, "ms_gpu": round(ms_total - ms_fmt, 3),
                    "ms_expand": ms_exp, "rank_pairs_per_s_expand": round(nodes / (ms_exp * 1e-3)) if ms_exp > 0 else None,
                    "nodes_per_s_gpu": round(nodes / ((ms_total - ms_fmt) * 1e-3)) if ms_total > ms_fmt else None})
    else:
        out["gpu_stderr_tail"] = (err or b"")[-400:].decode(errors="replace")
    if not a.no_ref and os.path.exists(REF):
        rwall, rrc, rmd5, rlines, _ = run_md5([REF] + args, a.ref_timeout)
        out.update({"ref_wall_s": round(rwall, 3) if rwall else None, "ref_rc": rrc, "ref_timed_out": rwall is None, "md5_match": rmd5 == md5 if rmd5 else None,
                    "speedup": round(rwall / wall, 1) if rwall and wall else None})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
