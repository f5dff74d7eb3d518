"""Timing of contact timelines (not a test): python tests/timeline_timing.py [--out FILE] [--reps N] [--label NAME] [--rings-freq-only] [--package DIR]

1ubq x 1000, 1ubq x 10 000 and 6bft x 1000 frames (seeded sigma = 0.3 A jitter), atom and residue level, rings off and on.  Warm, best of --reps
(default 10) calls: Context.contact_timelines, Context.contact_frequencies on the same arguments, their ratio; from the library's `timing` laps of
one timeline call (every lap ends in a stream synchronise) the split by sweep -- rows / marks / stats / download -- and, inside the mark sweep, the
laps of its passes (upload + tile + pair pass, ring fit, marks); for F = 100 at atom level without rings the per-frame Python loop that keeps the
frames (one atomic_contacts call per frame, the masks built in numpy) and the speed-up over it.  Prints one JSON line per case.
--rings-freq-only times contact_frequencies(rings=True) alone, 1ubq x 1000 and 6bft x 1000, --reps calls each in --series series (best of each
series): it uses nothing the timeline feature added, so with --package DIR (a tree that holds another build of the arpeggia_amd package) the same
file times an older tree's k_freq_ring_rows for an A/B in one session.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=10, type=int)
    ap.add_argument("--series", default=5, type=int)
    ap.add_argument("--label", default="")
    ap.add_argument("--rings-freq-only", action="store_true")
    ap.add_argument("--package", default=None)
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
        fn()  # (every call ends in the download of its table: the device has drained)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "max_ms": round(max(ts), 3), "repeats": reps}


def laps_of(fn) -> tuple:
    """The `timing` laps one call prints on stderr, summed by name (ms): (the timeline's sweeps, the laps of the frequency passes)."""
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
    sweeps, passes, in_marks = {}, {}, False
    for line in text.splitlines():
        line = line.strip()
        if not line.endswith(" ms"):
            continue
        for prefix, out in (("timeline ", sweeps), ("frequencies ", passes)):
            if line.startswith(prefix):
                name, ms = line[len(prefix):-3].rsplit(None, 1)
                if out is sweeps:
                    in_marks = name.strip() == "rows"  # (the frequency laps that follow belong to the mark sweep)
                    out[name.strip()] = out.get(name.strip(), 0.0) + float(ms)
                elif in_marks:
                    out[name.strip()] = out.get(name.strip(), 0.0) + float(ms)
    return sweeps, passes


def frame_loop(ctx, s, frames):
    """What a user has without this call: one atomic_contacts call per frame, the (row, frame) masks and their statistics in numpy."""
    import freq_residue_common as fc

    i, j, code, frame, _ = fc.atom_items(ctx, s, frames, "/")
    key = (i.astype(np.uint64) << np.uint64(34)) | (j.astype(np.uint64) << np.uint64(5)) | code.astype(np.uint64)
    uk, inv = np.unique(key, return_inverse=True)
    masks = np.zeros((len(uk), frames.shape[0]), bool)
    masks[inv, frame] = True
    starts = masks & ~np.concatenate([np.zeros((len(uk), 1), bool), masks[:, :-1]], 1)
    return len(uk), int(starts.sum())


def main():
    a = ARGS
    ctx = aa.Context(0)
    lines = []

    def emit(r):
        if a.label:
            r = dict(label=a.label, **r)
        print(json.dumps(r), flush=True)
        lines.append(r)

    if a.rings_freq_only:
        for name in ("1ubq", "6bft"):
            s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
            frames = frames_for(s, 1000, seed=1000)
            for _ in range(2):
                ctx.contact_frequencies(s, frames, rings=True)
            series = [timed(lambda: ctx.contact_frequencies(s, frames, rings=True), a.reps)["best_ms"] for _ in range(a.series)]
            emit({"structure": name, "frames": 1000, "call": "contact_frequencies(rings=True)", "best_ms_of_each_series": series, "reps_per_series": a.reps})
    else:
        for name, F in (("1ubq", 1000), ("1ubq", 10000), ("6bft", 1000)):
            s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
            frames = frames_for(s, F, seed=F)
            for level in ("atom", "residue"):
                for rings in (False, True):
                    r = {"structure": name, "frames": F, "atoms_per_frame": int(frames.shape[1]), "level": level, "rings": rings}
                    tl = lambda: ctx.contact_timelines(s, frames, "/", rings=rings, level=level)
                    fq = lambda: ctx.contact_frequencies(s, frames, "/", rings=rings, level=level)
                    for _ in range(2):
                        got = tl()
                        fq()
                    r["rows"] = int(len(got["n_frames"]))
                    r["bitmap_bytes"] = int(got["timeline_words"].nbytes)
                    r["timeline"] = timed(tl, a.reps)
                    r["frequencies"] = timed(fq, a.reps)
                    r["timeline_over_frequencies"] = round(r["timeline"]["best_ms"] / r["frequencies"]["best_ms"], 3)
                    r["no_bitmap"] = timed(lambda: ctx.contact_timelines(s, frames, "/", rings=rings, level=level, bitmap=False), a.reps)
                    sweeps, passes = laps_of(tl)
                    r["sweeps_ms"] = {k: round(v, 3) for k, v in sweeps.items()}
                    r["mark_sweep_laps_ms"] = {k: round(v, 3) for k, v in passes.items()}
                    emit(r)
            if F == 1000:  # F = 100: the per-frame loop a user has today
                f100 = frames[:100]
                frame_loop(ctx, s, f100[:10])
                loop = timed(lambda: frame_loop(ctx, s, f100), 3)
                for _ in range(2):
                    ctx.contact_timelines(s, f100, "/")
                call = timed(lambda: ctx.contact_timelines(s, f100, "/"), a.reps)
                emit({"structure": name, "frames": 100, "level": "atom", "rings": False, "loop": loop, "timeline": call,
                      "speedup_vs_loop": round(loop["best_ms"] / call["best_ms"], 2)})
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
