#!/usr/bin/env python3
"""BRE at scale, to be run once on the MI355X: the 64 M-symbol index of tools/probe_mem.py (K relatives of an L bp genome, both strands), then
  export  rb3gpu_export_bre at two length bytes beside rb3gpu_export_fmd_words on the same handle (wall of each call, ms_scan / ms_pack, pieces),
  import  rb3gpu_from_bre beside rb3gpu_from_fmd_words (wall of each call, ms_scan / ms_fill),
  cli     `build -e -i` and `mem -l31` on the .bre against the .fmd and against the reference binary, with md5.
One JSON line on stdout, also written to --out (profiles/bre_probe.json).
    python tools/probe_bre.py [--K 8] [--L 4000000] [--reads 200000] [--runs 3] [--workdir DIR] [--out FILE]"""
import argparse
import json
import os
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


def timed(fn, runs):
    walls, last = [], None
    for i in range(runs + 1):   # the first call is the warm-up
        t = time.perf_counter()
        last = fn()
        if i > 0:
            walls.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(walls), 3), last


def wall(cmd, timeout, runs=1):
    ws, last = [], None
    for _ in range(runs):
        last = run_md5(cmd, timeout)
        if last[0] is None or last[1] != 0:
            return {"rc": last[1], "timed_out": last[0] is None}
        ws.append(last[0])
    return {"wall_s": round(statistics.median(ws), 3), "rc": last[1], "md5": last[2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=4000000)
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/rb3_bre_probe")
    ap.add_argument("--timeout", type=float, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bre_probe.json"))
    a = ap.parse_args()
    from ropebwt3_amd import Rb3Gpu, gpu
    os.makedirs(a.workdir, exist_ok=True)
    fa, fmd, bre, q = (os.path.join(a.workdir, f) for f in ("rel.fa", "rel.fmd", "rel.bre", "reads.fa"))
    gen_family.relatives(a.K, a.L, fa)
    subprocess.run([CLI, "build", "-d", "-o", fmd, fa], check=True, stderr=subprocess.DEVNULL, timeout=a.timeout)
    g0 = gen_family.ALPH[np.random.default_rng(11).integers(0, 4, size=a.L)]
    write_reads(q, g0, a.reads, np.random.default_rng(31))
    out = {"probe": "bre", "K": a.K, "L": a.L, "n_symbols": 2 * a.K * a.L, "reads": a.reads, "runs": a.runs}

    h = Rb3Gpu(device=0, verbose=1)
    h.from_fmd_file(fmd)
    st = {}
    ms_fmd, words = timed(h.export_fmd_words, a.runs)
    ms_bre, rec = timed(lambda: h.export_bre(2, st), a.runs)
    out["export"] = {"ms_export_fmd_words": ms_fmd, "fmd_bytes": int(words.nbytes), "ms_export_bre": ms_bre, "bre_bytes": len(rec), "ms_scan": round(st["ms_scan"], 3), "ms_pack": round(st["ms_pack"], 3),
                     "n_rec": st["n_rec"], "n_run": st["n_run"], "n_pieces": st["n_pieces"], "bre_over_fmd": round(ms_bre / ms_fmd, 3),
                     "pack_GB_per_s": round(len(rec) / st["ms_pack"] / 1e6, 1) if st["ms_pack"] > 0 else None}
    counts = (st["n_rec"], st["n_sym"], st["n_run"])
    gpu.write_bre(bre, rec, 2, counts)
    raw = np.fromfile(fmd, dtype=np.uint8)
    mc = raw[32:80].view(np.uint64).astype(np.int64)
    fw = np.ascontiguousarray(raw[80:80 + int(raw[8:32].view(np.uint64)[1])]).view(np.uint64)
    ms_ffmd, _ = timed(lambda: h._chk(h._lib.rb3gpu_from_fmd_words(h._h, fw.size, fw.ctypes.data, mc.ctypes.data), "rb3gpu_from_fmd_words"), a.runs)
    plain = h.export_plain()
    si = {}
    ms_fbre, _ = timed(lambda: h.from_bre(rec, 2, si), a.runs)
    out["import"] = {"ms_from_fmd_words": ms_ffmd, "ms_from_bre": ms_fbre, "ms_scan": round(si["ms_scan"], 3), "ms_fill": round(si["ms_fill"], 3), "n_pieces": si["n_pieces"],
                     "same_index": bool(np.array_equal(h.export_plain(), plain)), "bre_over_fmd": round(ms_fbre / ms_ffmd, 3),
                     "fill_GB_per_s": round(si["n_sym"] / si["ms_fill"] / 1e6, 1) if si["ms_fill"] > 0 else None}
    h.close()

    cli = {"build_e_i": wall([CLI, "build", "-e", "-i", fmd], a.timeout, a.runs), "build_d_i": wall([CLI, "build", "-d", "-i", fmd], a.timeout, a.runs),
           "build_d_i_bre": wall([CLI, "build", "-d", "-i", bre], a.timeout, a.runs),
           "mem_fmd": wall([CLI, "mem", "-l31", fmd, q], a.timeout, a.runs), "mem_bre": wall([CLI, "mem", "-l31", bre, q], a.timeout, a.runs)}
    if os.path.exists(REF):
        cli["ref_build_e_i"] = wall([REF, "build", "-e", "-i", fmd], a.timeout)
        cli["ref_mem_bre_t16"] = wall([REF, "mem", "-t16", "-l31", bre, q], a.timeout)
        cli["md5_match"] = {"build_e": cli["ref_build_e_i"].get("md5") == cli["build_e_i"].get("md5"), "mem": cli["ref_mem_bre_t16"].get("md5") == cli["mem_bre"].get("md5")}
    cli["mem_bre_is_mem_fmd"] = cli["mem_bre"].get("md5") == cli["mem_fmd"].get("md5")
    cli["bre_file_is_build_e"] = cli["build_e_i"].get("md5") == __import__("hashlib").md5(open(bre, "rb").read()).hexdigest()
    out["cli"] = cli
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
