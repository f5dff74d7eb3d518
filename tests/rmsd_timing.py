"""Timing of the RMSD calls (not a test): python tests/rmsd_timing.py [--out FILE] [--reps N] [--cases 1ubq:ca:1000,...]

1ubq CA x 1000 and x 10 000 frames, 1ubq heavy atoms x 10 000, 6bft CA x 1000.  The frames are 40 states (the structure + a seeded sigma = 1.0 A step per
atom) with a seeded sigma = 0.3 A jitter per frame, each tumbled and shifted at random: an rmsd of about 0.7 A inside a state and 2.5 A between states, so
that a cutoff between the two gives a few dozen clusters.  Warm (two calls first), best of --reps (default 5) calls:
  matrix       Context.rmsd_matrix
  clusters     Context.rmsd_clusters at a cutoff between the two modes of the first 1000 frames' values
  reference    Context.rmsd against frame 0
  numpy_route  the route a user has without the calls, on the host's threads: centre, batched einsum covariances and a batched SVD in blocks of rows, then
               cluster_cases.gromos; its clustering is compared with the call's.  Measured once, and only up to --host-frames frames (default 1000: 10^6
               SVDs; 10^4 frames are 10^8)
  contact_clusters  Context.contact_clusters (atom level, min_similarity 0.5) on the same frames, as context; up to --host-frames frames
From the library's `timing` laps of one call each: the split pack (upload + k_rmsd_pack) / gram (k_rmsd_gram with its epilogue) / rounds / download.
Prints one JSON line per case.
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
import rmsd_cases as rc  # noqa: E402
import trajectory_shapes as ts  # noqa: E402

STATES = 40


def frames_for(s, F, seed):
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    base = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
    rng = np.random.default_rng(seed)
    states = base[None] + rng.normal(scale=1.0, size=(STATES, n, 3))
    out = states[rng.integers(0, STATES, F)] + rng.normal(scale=0.3, size=(F, n, 3))
    c = out.mean(1, keepdims=True)
    rot = np.stack([ts.random_rotation(rng) for _ in range(F)])
    return np.einsum("fia,fba->fib", out - c, rot) + c + rng.normal(scale=20.0, size=(F, 1, 3))


def timed(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # (every call ends in a download: the device has drained)
        t.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(t), 3), "median_ms": round(float(np.median(t)), 3), "max_ms": round(max(t), 3), "repeats": reps}


def laps_of(fn) -> dict:
    """The `timing` laps one call prints on stderr: {lap: ms}."""
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
        m = re.match(r"\s*rmsd (\S+)\s+([0-9.]+) ms", line)
        if m:
            laps[m.group(1)] = round(laps.get(m.group(1), 0.0) + float(m.group(2)), 3)
    return laps


def numpy_matrix(X, block=64):
    A, G = rc.centred(X)
    F, n = A.shape[:2]
    out = np.empty((F, F), np.float32)
    for f0 in range(0, F, block):
        S = np.einsum("fia,gib->fgab", A[f0:f0 + block], A)
        lam = rc.top_eigenvalue(S)
        out[f0:f0 + block] = np.sqrt(np.maximum(0.0, (G[f0:f0 + block, None] + G[None, :] - 2.0 * lam) / n))
    np.fill_diagonal(out, 0.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=5, type=int)
    ap.add_argument("--cases", default="1ubq:ca:1000,1ubq:ca:10000,1ubq:heavy:10000,6bft:ca:1000")
    ap.add_argument("--host-frames", default=1000, type=int)
    a = ap.parse_args()
    ctx = aa.Context(0)
    lines = []
    for name, atoms, F in [(c.split(":")[0], c.split(":")[1], int(c.split(":")[2])) for c in a.cases.split(",")]:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        sel = aa.rmsd_select(s, atoms)
        frames = frames_for(s, F, seed=F)
        head = ctx.rmsd_matrix(s, frames[:1000], atoms=sel)
        off = np.sort(head[~np.eye(len(head), dtype=bool)])
        gaps = np.diff(off)
        cutoff = float(off[int(np.argmax(gaps))] + 0.5 * gaps.max())   # the middle of the widest gap: between "same state" and "another state"
        calls = {"matrix": lambda: ctx.rmsd_matrix(s, frames, atoms=sel), "clusters": lambda: ctx.rmsd_clusters(s, frames, atoms=sel, cutoff=cutoff),
                 "reference": lambda: ctx.rmsd(s, frames, reference=0, atoms=sel)}
        r = {"structure": name, "atoms": atoms, "n": int(len(sel)), "frames": F, "atoms_per_frame": int(frames.shape[1]), "cutoff": round(cutoff, 4), "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()}
        for key, fn in calls.items():
            for _ in range(2):
                got = fn()
            r[key] = timed(fn, a.reps)
            r[key]["laps_ms"] = laps_of(fn)
            if key == "clusters":
                r["n_clusters"], r["largest_cluster"] = int(got["n_clusters"]), int(got["cluster_size"][0])
                clusters = got
        pairs = F * (F + 1) // 2
        r["gram_gflops_from_lap"] = round(pairs * 18 * (-(-len(sel) // 4) * 4) / (r["matrix"]["laps_ms"].get("gram", float("nan")) * 1e-3) / 1e9, 1)
        if F <= a.host_frames:
            X = frames[:, sel]
            t0 = time.perf_counter()
            m = numpy_matrix(X)
            t1 = time.perf_counter()
            cluster, centre, size = rc.gromos(m <= np.float32(cutoff))
            t2 = time.perf_counter()
            r["numpy_route"] = {"matrix_ms": round((t1 - t0) * 1e3, 1), "gromos_ms": round((t2 - t1) * 1e3, 1), "repeats": 1}
            r["numpy_route_equal"] = bool(np.array_equal(cluster, clusters["cluster"]) and np.array_equal(centre, clusters["centre"]))
            r["speedup_vs_numpy_route"] = round((t2 - t0) * 1e3 / r["clusters"]["best_ms"], 1)
            cc = lambda: ctx.contact_clusters(s, frames, "/", min_similarity=0.5, counts=False)
            cc()
            r["contact_clusters"] = timed(cc, 2)
        else:
            r["numpy_route"] = r["contact_clusters"] = "not measured"
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
