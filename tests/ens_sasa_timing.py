"""Timing of arp_sasa_ensemble (not a test): python tests/ens_sasa_timing.py [--out FILE] [--quick] [--profile]

For 1ubq x {100, 1000, 10 000} and 6bft x {100, 1000} frames (seeded sigma = 0.3 A jitter), SASA alone and with SAP: the call (warm; best and
median of the repeats) and the time per frame, against the per-frame Python loop of the existing calls (atom_sasa, and for SAP sap_weight +
sap_neighbor_sum) measured in the same run.  Prints one JSON line per case.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import arpeggia_amd as aa  # noqa: E402
import ens_sasa_common as ec  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, float(np.median(ts)) * 1e3


def loop_baseline(ctx, s, sel, frames, sap_radius):
    """What a user does today: one atom_sasa call per frame, for SAP also the weights and one sap_neighbor_sum call per frame; then numpy."""
    r = ec.vdw(s.strings("element")[sel])
    side = ~np.isin(s.strings("atomn")[sel], ec.BACKBONE)
    resn = [v.decode() for v in s.strings("resn")[sel]]
    counts, saps = [], []
    for f in range(frames.shape[0]):
        x, y, z = (np.ascontiguousarray(frames[f][sel, k]) for k in range(3))
        sasa, count = aa.atom_sasa(ctx, x, y, z, r, None, 1.4, 100)
        counts.append(count)
        if sap_radius is not None:
            w = np.array([aa.sap_weight(resn[k], float(sasa[k])) for k in range(len(sel))], np.float32)
            saps.append(aa.sap_neighbor_sum(ctx, x, y, z, side, w, sap_radius))
    c = np.array(counts)
    out = [c.mean(0), c.std(0), c.min(0), c.max(0)]
    if saps:
        p = np.array(saps)
        out += [p.mean(0), p.std(0)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--profile", action="store_true", help="only the calls (1ubq x 1000, 6bft x 1000 with SAP, 5 each): the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    ctx = aa.Context(0)
    if a.profile:
        for name in ("1ubq", "6bft"):
            s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
            frames = ec.jittered(s, 1000, seed=1000)
            for _ in range(5):
                ctx.sasa_ensemble(s, frames, sap_radius=5.0)
        return
    cases = [("1ubq", 100), ("1ubq", 1000), ("1ubq", 10000), ("6bft", 100), ("6bft", 1000)]
    if a.quick:
        cases = [("1ubq", 100), ("1ubq", 1000)]
    lines = []
    for name, F in cases:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        frames = ec.jittered(s, F, seed=F)
        sel = aa.sasa_select(s)
        for sap_radius in (None, 5.0):
            reps = 10 if F * len(sel) <= 1_000_000 else 3
            ctx.sasa_ensemble(s, frames, sap_radius=sap_radius)  # warm: workspace, buffers
            best, med = timed(lambda: ctx.sasa_ensemble(s, frames, sap_radius=sap_radius), reps)
            # the loop on every frame up to 1000; beyond that on the first 1000, scaled to F (every frame is the same work)
            Fl = min(F, 1000)
            loop_baseline(ctx, s, sel, frames[: min(F, 10)], sap_radius)  # warm
            lb, lm = timed(lambda: loop_baseline(ctx, s, sel, frames[:Fl], sap_radius), 3 if Fl * len(sel) <= 200_000 else 1)
            r = {"structure": name, "frames": F, "selected_atoms": int(len(sel)), "with_sap": sap_radius is not None, "call_best_ms": round(best, 3),
                 "call_median_ms": round(med, 3), "us_per_frame": round(best * 1e3 / F, 3), "loop_frames_measured": Fl,
                 "loop_us_per_frame": round(lb * 1e3 / Fl, 3), "loop_best_ms_scaled_to_F": round(lb * F / Fl, 3),
                 "speedup_vs_loop": round(lb * F / Fl / best, 2)}
            print(json.dumps(r), flush=True)
            lines.append(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
