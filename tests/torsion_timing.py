"""Timing of the torsion call (not a test): python tests/torsion_timing.py [--out FILE] [--reps N] [--cases 1ubq:1000,...] [--no-host]

1ubq x 1000 and x 10 000 frames, 6bft x 100 and x 1000 frames: the file's atoms with a seeded 0.3 A jitter per atom and frame.  Warm (two calls first), then
--reps calls (default 5), best / median / max:
  call          Context.torsions(angles=True, bins=36, rama="class") from the frames in host memory to the result in host memory
  laps_ms       the library's `timing` laps of one call, added up over the upload passes: upload, angle (k_torsion_angle + k_torsion_slab), hist (k_torsion_hist
                + the Ramachandran maps), finish (k_torsion_sums + k_torsion_stats), download; each one's share of their sum; the upload's share
  angle         F D samples over the angle lap: samples per second
  hist_routes   the hist lap (best of three calls) of the same input with the maps of the four classes on each route -- "lds" (the default at 4 x 36 x 36),
                "matched" (wave-matched global adds), "plain" (one global add per sample) -- and with one map per residue ("residue": matched, the route of
                tables beyond LDS; "residue_plain": one global add per sample); so the cost of contention is on record
  host          arp_torsions_host over the same frames, gathered by torsion_select, split over 16 processes (spawned, no device), wall time of the pool's map with
                the workers already started; and whether the counts that add up over a split of the frames (state_counts, hist, hist2) equal the device's
Prints one JSON line per case.
"""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import os
import re
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT / "tests"), str(ROOT)):
    if p in sys.path:
        sys.path.remove(p)
    sys.path.insert(0, p)

HOST_PROCESSES = 16


def host_part(args):
    import arpeggia_amd as aa

    quad_xyz, pairs = args
    res = aa.torsions_host(quad_xyz, pairs, 4, 36, angles=True, cossin=False, states=False)
    return {k: res[k] for k in ("state_counts", "hist", "hist2")}


def warm(_):
    import arpeggia_amd  # noqa: F401

    return os.getpid()


def laps_of(aa, fn) -> dict:
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            aa.debug_set("timing", 1)
            fn()
        finally:
            aa.debug_set("timing", 0)
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    laps = {}
    for line in text.splitlines():
        m = re.match(r"\s*torsions (\S+)\s+([0-9.]+) ms", line)
        if m:
            laps[m.group(1)] = round(laps.get(m.group(1), 0.0) + float(m.group(2)), 3)
    return laps


def timed(fn, reps: int) -> dict:
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # (the call ends in a download: the device has drained)
        t.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(t), 3), "median_ms": round(float(np.median(t)), 3), "max_ms": round(max(t), 3), "repeats": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=5, type=int)
    ap.add_argument("--cases", default="1ubq:1000,1ubq:10000,6bft:100,6bft:1000")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    a = ap.parse_args()
    pool = None
    if not a.no_host:
        pool = mp.get_context("spawn").Pool(HOST_PROCESSES)   # started before the device is opened; the workers never open it
        pool.map(warm, range(HOST_PROCESSES * 4))
    import arpeggia_amd as aa
    import trajectory_shapes as ts

    ctx = aa.Context(0)
    lines = []
    for name, F in [(c.split(":")[0], int(c.split(":")[1])) for c in a.cases.split(",")]:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        n = aa.api._topology_atoms(s)
        soa = s.soa("/")
        base = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
        frames = ts.jitter(base, F, seed=F)
        sel = aa.torsion_select(s)
        D, P = int(len(sel["quads"])), int(len(sel["pairs"]))
        call = lambda rama="class": ctx.torsions(s, frames, rama=rama)
        for _ in range(2):
            got = call()
        r = {"structure": name, "frames": F, "torsions": D, "pairs": P, "residues": int(sel["n_rows"]), "atoms_per_frame": n, "call": timed(call, a.reps),
             "laps_ms": laps_of(aa, call)}
        total = sum(r["laps_ms"].values())
        r["lap_share"] = {k: round(v / total, 4) for k, v in r["laps_ms"].items()} if total else {}
        r["upload_share"] = r["lap_share"].get("upload")
        angle_ms = r["laps_ms"].get("angle")
        if angle_ms:
            r["angle"] = {"samples": F * D, "lap_ms": angle_ms, "samples_per_s": round(F * D / (angle_ms * 1e-3), 1)}
        routes = {}
        for label, route, rama in (("lds", 1, "class"), ("matched", 2, "class"), ("plain", 3, "class"), ("residue", 0, "residue"), ("residue_plain", 3, "residue")):
            aa.debug_set("torsion_hist2_route", route)
            try:
                fn = lambda: call(rama)
                fn()
                routes[label] = min(laps_of(aa, fn).get("hist", float("nan")) for _ in range(3))
            finally:
                aa.debug_set("torsion_hist2_route", 0)
        r["hist_routes_ms"] = routes
        if pool is None:
            print(json.dumps(r), flush=True)
            lines.append(r)
            continue
        qx = frames[:, sel["quads"].astype(np.int64)]
        parts = [(qx[k::HOST_PROCESSES], sel["pairs"]) for k in range(HOST_PROCESSES) if len(qx[k::HOST_PROCESSES])]
        t, host = [], None
        for _ in range(max(2, a.reps // 2)):
            t0 = time.perf_counter()
            host = pool.map(host_part, parts)
            t.append((time.perf_counter() - t0) * 1e3)
        r["host"] = {"processes": len(parts), "best_ms": round(min(t), 3), "median_ms": round(float(np.median(t)), 3), "max_ms": round(max(t), 3), "repeats": len(t)}
        r["equal_to_host"] = bool(all(np.array_equal(sum(p[k].astype(np.uint64) for p in host), got[k]) for k in ("state_counts", "hist", "hist2")))
        r["speedup_vs_host"] = round(r["host"]["best_ms"] / r["call"]["best_ms"], 2)
        r["spreads_apart"] = r["call"]["max_ms"] < r["host"]["best_ms"]
        print(json.dumps(r), flush=True)
        lines.append(r)
    if pool is not None:
        pool.close()
        pool.join()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
