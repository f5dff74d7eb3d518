"""Timing of the buried-surface calls (not a test): python tests/bsa_timing.py [--out FILE] [--quick]

Single structure, warm, best and median of the repeats, the two calls alternating: Context.buried_sasa (one walk of k_sasa_split over the union,
per-atom and per-residue tables, the total) against get_dsasa (the three-model packing of k_sasa, the scalar only), on 6bft "C/H,L" and on a
10^5-atom S1 cloud whose template copies alternate between two chains.  Ensemble: Context.dsasa_ensemble on 1ubq x 1000 ("/") and 6bft x 1000
("C/H,L") frames (seeded sigma = 0.3 A jitter) against a per-frame loop of get_dsasa on structures built from each frame's coordinates; the loop
runs over the first LOOP_FRAMES frames, the structures are built outside the timed window, and both are reported per frame.  Both sides end in
a device synchronise (the calls are synchronous).  Prints one JSON line per case.
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
import synth  # noqa: E402

LOOP_FRAMES = 100


def alternating(fns: dict, reps: int) -> dict:
    """Every function `reps` times, one after the other in turn; per function (best, median) in ms."""
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: (round(min(v) * 1e3, 3), round(float(np.median(v)) * 1e3, 3)) for k, v in ts.items()}


def two_chain_cloud(n_atoms: int) -> aa.Structure:
    rec = synth.gen_s1(n_atoms)
    copy = np.unique(rec["chain"], return_inverse=True)[1]
    rec["chain"] = np.where(copy % 2 == 0, b"A", b"B").astype("S8")
    return aa.Structure.from_records(rec, hierarchy=True)


def single(ctx, name: str, s: aa.Structure, groups: str, reps: int) -> dict:
    for _ in range(3):  # warm: workspace, buffers, code objects
        new, old = ctx.buried_sasa(s, groups), aa.get_dsasa(s, groups)
    assert np.float32(new["dsasa"]) == np.float32(old), (new["dsasa"], old)
    t = alternating({"split": lambda: ctx.buried_sasa(s, groups), "packed": lambda: aa.get_dsasa(s, groups)}, reps)
    return {"case": "single", "structure": name, "groups": groups, "atoms": len(new["atoms"]), "dsasa": float(old),
            "buried_sasa_best_ms": t["split"][0], "buried_sasa_median_ms": t["split"][1], "get_dsasa_best_ms": t["packed"][0],
            "get_dsasa_median_ms": t["packed"][1], "ratio_best": round(t["packed"][0] / t["split"][0], 3)}


def frame_structures(name: str, frames: np.ndarray) -> list:
    rec = synth.read_pdb_records(ROOT / "tests" / "data" / f"{name}.pdb")
    top = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
    sel = np.searchsorted(rec["serial"], top.ints("atomi"))
    out = []
    for f in range(len(frames)):
        r = {k: v[sel].copy() for k, v in rec.items()}
        r["x"], r["y"], r["z"] = (np.ascontiguousarray(frames[f, :, c]) for c in range(3))
        out.append(aa.Structure.from_records(r))
    return out


def ensemble(ctx, name: str, groups: str, F: int, reps: int) -> dict:
    s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    base = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
    frames = base[None] + np.random.default_rng(F).normal(scale=0.3, size=(F, n, 3))
    got = ctx.dsasa_ensemble(s, frames, groups)  # warm
    structures = frame_structures(name, frames[:LOOP_FRAMES])
    loop = [aa.get_dsasa(q, groups) for q in structures]  # warm
    same = bool(np.array_equal(np.array(loop, np.float32), got["dsasa"][: len(loop)]))
    t = alternating({"ens": lambda: ctx.dsasa_ensemble(s, frames, groups), "loop": lambda: [aa.get_dsasa(q, groups) for q in structures]}, reps)
    return {"case": "ensemble", "structure": name, "groups": groups, "frames": F, "atoms_per_frame": len(got["atoms"]), "loop_frames": len(structures),
            "loop_equals_ensemble": same, "ensemble_best_ms": t["ens"][0], "ensemble_median_ms": t["ens"][1],
            "ensemble_us_per_frame": round(t["ens"][0] * 1e3 / F, 3), "loop_best_ms": t["loop"][0], "loop_median_ms": t["loop"][1],
            "loop_us_per_frame": round(t["loop"][0] * 1e3 / len(structures), 3),
            "per_frame_ratio": round((t["loop"][0] / len(structures)) / (t["ens"][0] / F), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    ctx = aa.Context(0)
    lines = []

    def emit(r):
        print(json.dumps(r), flush=True)
        lines.append(r)

    emit(single(ctx, "6bft", aa.load_model(str(ROOT / "tests" / "data" / "6bft.pdb")), "C/H,L", 30))
    if not a.quick:
        emit(single(ctx, "s1_100k", two_chain_cloud(100_000), "A/B", 15))
    emit(ensemble(ctx, "1ubq", "/", 100 if a.quick else 1000, 5))
    if not a.quick:
        emit(ensemble(ctx, "6bft", "C/H,L", 1000, 3))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
