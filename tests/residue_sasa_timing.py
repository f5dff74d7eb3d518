"""Timing of the residue level (not a test): python tests/residue_sasa_timing.py [--out FILE] [--frames F] [--profile NAME]

Warm, best of 10, one JSON line per case:
  (a) get_residue_sasa against get_atom_sasa on 1ubq and 6bft;
  (b) get_residue_sasa_ensemble on 1ubq x F and 6bft x F (default 1000; seeded sigma = 0.3 A jitter) against two calls that predate it:
      (i)  get_sasa_ensemble without per-frame output -- the floor: the same k_sasa work;
      (ii) get_sasa_ensemble(per_frame=True) plus a numpy group-by per residue -- what a user did before.
--profile 1ubq|6bft: only five residue-ensemble calls on that input, the run to put under rocprofv3 --kernel-trace --stats.
Default output: profiles/r12_residue_sasa_timing.jsonl.
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

FOUR_PI = 4.0 * 3.141592653589793


def best_ms(fn, reps=10):
    fn()  # warm: workspace, buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(min(ts) * 1e3, 3), round(float(np.median(ts)) * 1e3, 3)


def group_by_residue(s, frames, ids, R):
    """Baseline (ii): the per-frame counts of every atom come to the host, numpy turns them into areas and sums them per residue."""
    _, extras = aa.get_sasa_ensemble(s, frames, per_frame=True)
    sasa = ((FOUR_PI * R * R)[None] * extras["count"] / 100.0).astype(np.float32)
    per_res = np.stack([np.bincount(ids, weights=row, minlength=ids.max() + 1) for row in sasa.astype(np.float64)])
    return per_res.mean(0), per_res.std(0), per_res.min(0), per_res.max(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12_residue_sasa_timing.jsonl"))
    ap.add_argument("--frames", default=1000, type=int)
    ap.add_argument("--profile", default=None, choices=("1ubq", "6bft"))
    a = ap.parse_args()
    if a.profile:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{a.profile}.pdb"))
        frames = ec.jittered(s, a.frames, seed=a.frames)
        for _ in range(5):
            aa.get_residue_sasa_ensemble(s, frames)
        return
    lines = []
    for name in ("1ubq", "6bft"):
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        sel = aa.sasa_select(s)
        atom, atom_med = best_ms(lambda: aa.get_atom_sasa(s))
        res, res_med = best_ms(lambda: aa.get_residue_sasa(s))
        chain, _ = best_ms(lambda: aa.get_chain_sasa(s))
        lines.append({"case": "single", "structure": name, "selected_atoms": int(len(sel)), "get_atom_sasa_best_ms": atom, "get_atom_sasa_median_ms": atom_med,
                      "get_residue_sasa_best_ms": res, "get_residue_sasa_median_ms": res_med, "get_chain_sasa_best_ms": chain})
        print(json.dumps(lines[-1]), flush=True)
        frames = ec.jittered(s, a.frames, seed=a.frames)
        key = np.stack([s.strings("chain")[sel], s.ints("resi")[sel].astype("S12"), s.strings("insertion")[sel]], 1)
        ids = np.unique(key, axis=0, return_inverse=True)[1].reshape(-1)
        R = (ec.vdw(s.strings("element")[sel]) + np.float32(1.4)).astype(np.float64)
        reps = 10
        res_ens, res_ens_med = best_ms(lambda: aa.get_residue_sasa_ensemble(s, frames), reps)
        floor, floor_med = best_ms(lambda: aa.get_sasa_ensemble(s, frames), reps)
        today, today_med = best_ms(lambda: group_by_residue(s, frames, ids, R), reps)
        lines.append({"case": "ensemble", "structure": name, "frames": a.frames, "selected_atoms": int(len(sel)), "repeats": reps,
                      "get_residue_sasa_ensemble_best_ms": res_ens, "get_residue_sasa_ensemble_median_ms": res_ens_med,
                      "floor_get_sasa_ensemble_best_ms": floor, "floor_get_sasa_ensemble_median_ms": floor_med,
                      "per_frame_plus_numpy_group_by_best_ms": today, "per_frame_plus_numpy_group_by_median_ms": today_med,
                      "over_floor": round(res_ens / floor, 3), "speedup_vs_group_by": round(today / res_ens, 2)})
        print(json.dumps(lines[-1]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
