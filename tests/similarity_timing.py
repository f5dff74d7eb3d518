"""Timing of contact similarity (not a test): python tests/similarity_timing.py [--out FILE] [--reps N] [--label NAME] [--timelines-only] [--package DIR]

1ubq x 1000, 1ubq x 10 000 and 6bft x 1000 frames (seeded sigma = 0.3 A jitter), atom and residue level.  Warm, best of --reps (default 5) calls:
  similarity   Context.contact_similarity (between frames, Tanimoto)
  timelines    Context.contact_timelines(bitmap=False) on the same arguments: what the call costs on top of the sweeps it shares
  host_route   what a user has without the call: contact_timelines(bitmap=True) + unpack_timeline + a numpy Gram (f32 BLAS matmul, exact below 2^24
               rows) + the Tanimoto formula in f64 -> f32; its matrix is compared with the call's for equal bytes.  Timed once beyond 1000 frames.
From the library's `timing` laps of one similarity call: the split rows / marks / transpose / gram / download, and the time of k_bit_gram alone from
device events with its rate in word pairs per second (M x M x K per launch: the kernel computes the upper tile triangle, so the rate it sustains
on the pairs it touches is about twice that).  Prints one JSON line per case.
--timelines-only times contact_timelines alone (bitmap on and off), --reps calls in each of --series series: it uses nothing the similarity feature
added, so with --package DIR (a tree that holds another build of the arpeggia_amd package) the same file times an older tree for an A/B in one session.
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


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=5, type=int)
    ap.add_argument("--series", default=3, type=int)
    ap.add_argument("--label", default="")
    ap.add_argument("--timelines-only", action="store_true")
    ap.add_argument("--package", default=None)
    ap.add_argument("--cases", default="1ubq:1000,1ubq:10000,6bft:1000")
    return ap.parse_args()


ARGS = _args()
for p in (str(ROOT / "tests"), ARGS.package or str(ROOT)):
    if p in sys.path:
        sys.path.remove(p)
    sys.path.insert(0, p)

import arpeggia_amd as aa  # noqa: E402


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


def laps_of(fn) -> tuple:
    """The `timing` laps one similarity call prints on stderr: ({lap: ms}, k_bit_gram ms from events or None)."""
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
    laps, kernel = {}, None
    for line in text.splitlines():
        m = re.match(r"\s*similarity (\S+)\s+([0-9.]+) ms", line)
        if m and m.group(1) == "k_bit_gram":
            kernel = float(m.group(2))
        elif m:
            laps[m.group(1)] = laps.get(m.group(1), 0.0) + float(m.group(2))
    return laps, kernel


def host_route(ctx, s, frames, level):
    tl = ctx.contact_timelines(s, frames, "/", level=level, bitmap=True)
    sets = aa.unpack_timeline(tl["timeline_words"], frames.shape[0]).T.astype(np.float32)
    inter = sets @ sets.T
    sizes = np.diag(inter).copy()
    union = sizes[:, None].astype(np.float64) + sizes[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        sim = (inter.astype(np.float64) / union).astype(np.float32)
    sim[union == 0] = 1.0
    return sim


def main():
    a = ARGS
    ctx = aa.Context(0)
    lines = []

    def emit(r):
        if a.label:
            r = dict(label=a.label, **r)
        print(json.dumps(r), flush=True)
        lines.append(r)

    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in a.cases.split(",")]
    for name, F in cases:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        frames = frames_for(s, F, seed=F)
        for level in ("atom", "residue"):
            r = {"structure": name, "frames": F, "atoms_per_frame": int(frames.shape[1]), "level": level}
            if a.timelines_only:
                for bitmap in (True, False):
                    fn = lambda: ctx.contact_timelines(s, frames, "/", level=level, bitmap=bitmap)
                    for _ in range(2):
                        fn()
                    r["bitmap" if bitmap else "no_bitmap"] = [timed(fn, a.reps)["best_ms"] for _ in range(a.series)]
                r["call"] = "contact_timelines, best ms of each series"
                emit(r)
                continue
            sim = lambda: ctx.contact_similarity(s, frames, "/", level=level)
            tl = lambda: ctx.contact_timelines(s, frames, "/", level=level, bitmap=False)
            for _ in range(2):
                got = sim()
                tl()
            r["rows"] = int(len(got["n_frames"]))
            r["matrix_bytes"] = int(got["similarity"].nbytes)
            r["similarity"] = timed(sim, a.reps)
            r["timelines_no_bitmap"] = timed(tl, a.reps)
            r["similarity_over_timelines"] = round(r["similarity"]["best_ms"] / r["timelines_no_bitmap"]["best_ms"], 3)
            laps, kernel = laps_of(sim)
            r["laps_ms"] = {k: round(v, 3) for k, v in laps.items()}
            K = (r["rows"] + 31) // 32
            if kernel:
                r["k_bit_gram_ms"] = round(kernel, 4)
                r["k_bit_gram_words_K"] = K
                r["k_bit_gram_gwordpairs_per_s"] = round(F * F * K / (kernel * 1e-3) / 1e9, 2)
            host_reps = a.reps if F <= 1000 else 1
            if F <= 1000:
                host_route(ctx, s, frames, level)
            t0 = time.perf_counter()
            want = host_route(ctx, s, frames, level)
            first = (time.perf_counter() - t0) * 1e3
            r["host_route"] = timed(lambda: host_route(ctx, s, frames, level), host_reps) if host_reps > 1 else {"best_ms": round(first, 3), "repeats": 1}
            r["host_route_equal_bytes"] = bool(want.tobytes() == got["similarity"].tobytes())
            r["speedup_vs_host_route"] = round(r["host_route"]["best_ms"] / r["similarity"]["best_ms"], 2)
            emit(r)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
