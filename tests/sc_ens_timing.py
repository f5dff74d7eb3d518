"""Timing of shape complementarity across frames (not a test): python tests/sc_ens_timing.py [--out FILE] [--quick]

get_sc_ensemble (every frame of a pass in one set of launches; frame and atom tables included) against the per-frame loop of get_sc_results on
structures built from each frame's coordinates, on the same device, warm, the two alternating, for 1ubq cut into two chains (residues 1-38 /
39-76, "A/B") and 6bft "H/L", each x 100 and x 1000 frames (seeded sigma = 0.2 A jitter of model 0).  The loop runs over the first LOOP_FRAMES
frames with its structures built outside the timed window; both sides are reported per frame, the loop with the spread of its repeats.  The
stage laps are the profiler's, of one pass of LAP_FRAMES frames (arp_debug_set "sc_ens_frames"), next to the laps of one single-frame call.
Prints one JSON line per case."""
from __future__ import annotations

import argparse
import ctypes as C
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
from arpeggia_amd import _lib  # noqa: E402

LOOP_FRAMES = 100
LAP_FRAMES = 32


def records(name: str) -> dict:
    rec = synth.read_pdb_records(ROOT / "tests" / "data" / f"{name}.pdb")
    top = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
    sel = np.searchsorted(rec["serial"], top.ints("atomi"))
    rec = {k: v[sel].copy() for k, v in rec.items()}
    if name == "1ubq":
        rec["chain"] = np.where(rec["resi"] <= 38, b"A", b"B").astype("S8")
    return rec


def laps(ctx) -> dict:
    """The profiler's laps, laps of one name summed (ms)."""
    names, ms = (C.c_char_p * 32)(), (C.c_float * 32)()
    k = _lib.lib.arp_profile_read(ctx._h, names, ms, 32)
    out = {}
    for i in range(k):
        out[names[i].decode()] = round(out.get(names[i].decode(), 0.0) + float(ms[i]), 4)
    return out


def case(name: str, groups: str, F: int, reps: int) -> dict:
    rec = records(name)
    s = aa.Structure.from_records(rec)
    base = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    frames = base[None] + np.random.default_rng(F).normal(scale=0.2, size=(F, len(base), 3))
    frames[0] = base
    structures = []
    for f in range(min(F, LOOP_FRAMES)):
        r = dict(rec)
        r["x"], r["y"], r["z"] = (np.ascontiguousarray(frames[f, :, c]) for c in range(3))
        structures.append(aa.Structure.from_records(r))
    ft, at = aa.get_sc_ensemble(s, frames, groups)  # warm
    loop = [aa.get_sc_results(q, groups)["sc"] for q in structures]  # warm
    ft = ft if hasattr(ft, "column_names") else ft.to_arrow()
    same = loop == ft.column("sc").to_pylist()[: len(loop)]
    t_ens, t_loop = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        aa.get_sc_ensemble(s, frames, groups)
        t_ens.append((time.perf_counter() - t0) / F)
        t0 = time.perf_counter()
        for q in structures:
            aa.get_sc_results(q, groups)
        t_loop.append((time.perf_counter() - t0) / len(structures))
    ctx = aa.api._context(0)
    ctx.profile(True)
    aa.debug_set("sc_ens_frames", min(F, LAP_FRAMES))
    ctx.sc_ensemble(s, frames[: min(F, LAP_FRAMES)], groups)
    ens_laps = laps(ctx)
    aa.debug_set("sc_ens_frames", 0)
    aa.get_sc_results(structures[0], groups)
    one_laps = laps(ctx)
    ctx.profile(False)
    us = lambda v: round(v * 1e6, 1)
    return {"case": "sc_ensemble", "structure": name, "groups": groups, "frames": F, "atoms_per_frame": at.num_rows if hasattr(at, "num_rows") else len(at),
            "loop_frames": len(structures), "sc_equal_to_loop": bool(same), "frames_ok": int(sum(k == "ok" for k in ft.column("status").to_pylist())),
            "ensemble_us_per_frame_best": us(min(t_ens)), "ensemble_us_per_frame_max": us(max(t_ens)),
            "loop_us_per_frame_best": us(min(t_loop)), "loop_us_per_frame_median": us(float(np.median(t_loop))), "loop_us_per_frame_max": us(max(t_loop)),
            "per_frame_ratio_best": round(min(t_loop) / min(t_ens), 2), "per_frame_ratio_worst": round(min(t_loop) / max(t_ens), 2),
            "lap_frames": min(F, LAP_FRAMES), "ensemble_pass_laps_ms": ens_laps, "single_call_laps_ms": one_laps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    lines = []
    for name, groups in (("1ubq", "A/B"), ("6bft", "H/L")):
        for F in ((20,) if a.quick else (100, 1000)):
            r = case(name, groups, F, 3)
            print(json.dumps(r), flush=True)
            lines.append(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
