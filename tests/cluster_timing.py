"""Timing of contact clusters (not a test): python tests/cluster_timing.py [--out FILE] [--reps N] [--cases 1ubq:1000,...]

1ubq x 1000, 1ubq x 10 000 and 6bft x 1000 frames (seeded sigma = 0.3 A jitter), atom and residue level, at two thresholds taken from the similarities of the
first 1000 frames: their median (a few clusters) and their 99.9th percentile (hundreds at 1000 frames, thousands at 10 000).  Warm, best of --reps (default 5)
calls:
  clusters     Context.contact_clusters
  timelines    Context.contact_timelines(bitmap=False) on the same arguments: the floor, the sweeps every ensemble call shares
  similarity   Context.contact_similarity on the same arguments: the first half of the route a user has without the call
  host_route   that route whole: contact_similarity + the numpy thresholding and loop of tests/cluster_cases.py (f32 BLAS for the counts); its assignment is
               compared with the call's for equality.  Timed once beyond 1000 frames, and left out ("not measured") where clusters x frames^2 exceeds
               --host-limit: the loop reads the whole matrix once per cluster.
From the library's `timing` laps of one clusters call: the split rows / marks / transpose / adjacency / rounds / counts / download.  Prints one JSON line per
case and threshold.
"""
from __future__ import annotations

import argparse
import json
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

import arpeggia_amd as aa  # noqa: E402
import cluster_cases as cc  # noqa: E402


def frames_for(s, F, seed):
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    base = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
    return base[None] + np.random.default_rng(seed).normal(scale=0.3, size=(F, n, 3))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # (every call ends in a download: the device has drained)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "max_ms": round(max(ts), 3), "repeats": reps}


def laps_of(fn) -> dict:
    """The `timing` laps one clusters call prints on stderr: {lap: ms}."""
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
        m = re.match(r"\s*clusters (\S+)\s+([0-9.]+) ms", line)
        if m:
            laps[m.group(1)] = laps.get(m.group(1), 0.0) + float(m.group(2))
    return laps


def host_route(ctx, s, frames, level, thr):
    sim = ctx.contact_similarity(s, frames, "/", level=level)["similarity"]
    return cc.gromos(sim >= np.float32(thr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=5, type=int)
    ap.add_argument("--cases", default="1ubq:1000,1ubq:10000,6bft:1000")
    ap.add_argument("--host-limit", default=6e10, type=float, help="the host route is left out where clusters x frames^2 exceeds this")
    a = ap.parse_args()
    ctx = aa.Context(0)
    lines = []
    for name, F in [(c.split(":")[0], int(c.split(":")[1])) for c in a.cases.split(",")]:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        frames = frames_for(s, F, seed=F)
        for level in ("atom", "residue"):
            head = ctx.contact_similarity(s, frames[:1000], "/", level=level)["similarity"]
            off = np.sort(head[~np.eye(len(head), dtype=bool)])
            tl = lambda: ctx.contact_timelines(s, frames, "/", level=level, bitmap=False)
            sim = lambda: ctx.contact_similarity(s, frames, "/", level=level)
            for _ in range(2):
                tl()
                sim()
            floor, matrix = timed(tl, a.reps), timed(sim, a.reps)
            for what, q in (("few", 0.5), ("many", 0.999)):
                thr = float(off[int(q * (len(off) - 1))])
                call = lambda: ctx.contact_clusters(s, frames, "/", level=level, min_similarity=thr)
                for _ in range(2):
                    got = call()
                r = {"structure": name, "frames": F, "atoms_per_frame": int(frames.shape[1]), "level": level, "rows": int(len(got["n_frames"])), "threshold": what,
                     "min_similarity": thr, "n_clusters": int(got["n_clusters"]), "largest_cluster": int(got["cluster_size"][0]), "clusters": timed(call, a.reps),
                     "timelines_no_bitmap": floor, "similarity": matrix}
                r["laps_ms"] = {k: round(v, 3) for k, v in laps_of(call).items()}
                r["clusters_over_timelines"] = round(r["clusters"]["best_ms"] / floor["best_ms"], 3)
                if r["n_clusters"] * F * F > a.host_limit:  # (the numpy loop reads the whole matrix once per cluster)
                    r["host_route"] = "not measured"
                else:
                    host_reps = a.reps if F <= 1000 else 1
                    t0 = time.perf_counter()
                    cluster, centre, size = host_route(ctx, s, frames, level, thr)
                    first = (time.perf_counter() - t0) * 1e3
                    r["host_route"] = timed(lambda: host_route(ctx, s, frames, level, thr), host_reps) if host_reps > 1 else {"best_ms": round(first, 3), "repeats": 1}
                    r["host_route_equal"] = bool(np.array_equal(cluster, got["cluster"]) and np.array_equal(centre, got["centre"]) and np.array_equal(size, got["cluster_size"]))
                    r["speedup_vs_host_route"] = round(r["host_route"]["best_ms"] / r["clusters"]["best_ms"], 2)
                print(json.dumps(r), flush=True)
                lines.append(r)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
