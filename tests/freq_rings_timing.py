"""Timing of the ring rows of contact frequencies (not a test): python tests/freq_rings_timing.py [--out FILE] [--off-only] [--label NAME]

1ubq x 1000 and 6bft x 1000 frames (seeded sigma = 0.3 A jitter), rings off and on: the warm call (best, median, minimum and maximum of the
repeats), the ratio on / off, and -- from the library's `timing` laps of one call, every lap ending in a stream synchronise -- the share of the two
ring kernels (k_freq_ring_fit, k_freq_ring_rows) in that call's device pipeline.  For F = 100: the loop a user has without this feature, one
Structure.from_records + get_contacts per frame, and the speed-up over it.  One synthetic topology of about 10^5 atoms (synth.gen_stress at
protein density, residues of 6bft) x 20 frames, rings off and on: the price of the brute-force ring - cation sweep where it is weakest.
--off-only runs the rings-off calls alone and uses nothing this feature added: the same file runs against an older tree's package for an A/B
in one session.  Prints one JSON line per case.
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
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import arpeggia_amd as aa  # noqa: E402
import synth  # noqa: E402


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
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "repeats": reps}


def laps_of(fn) -> dict:
    """The `timing` laps one call prints on stderr, summed by name (ms)."""
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
    out = {}
    for line in text.splitlines():
        line = line.strip()
        if line.startswith("frequencies ") and line.endswith(" ms"):
            name, ms = line[len("frequencies "):-3].rsplit(None, 1)
            out[name.strip()] = out.get(name.strip(), 0.0) + float(ms)
    return out


def frame_loop(ctx, rec, frames):
    """What a user has without ring rows in the frequency table: one single-model structure and one get_contacts per frame."""
    rows = 0
    for f in range(frames.shape[0]):
        s = aa.Structure.from_records(dict(rec, x=frames[f, :, 0].copy(), y=frames[f, :, 1].copy(), z=frames[f, :, 2].copy()))
        t = ctx.get_contacts(s, "/", 0.1, 6.5)
        rows += int(((t["from_atom"] < 0) | (t["to_atom"] < 0)).sum())
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    ctx = aa.Context(0)
    lines = []

    def emit(r):
        if a.label:
            r = dict(label=a.label, **r)
        print(json.dumps(r), flush=True)
        lines.append(r)

    for name in ("1ubq", "6bft"):
        path = ROOT / "tests" / "data" / f"{name}.pdb"
        s = aa.load_model(str(path))
        frames = frames_for(s, 1000, seed=1000)
        r = {"structure": name, "frames": 1000, "atoms_per_frame": int(frames.shape[1])}
        for _ in range(2):
            ctx.contact_frequencies(s, frames)  # warm: workspace, buffers
        r["rings_off"] = timed(lambda: ctx.contact_frequencies(s, frames), 10)
        if not a.off_only:
            for _ in range(2):
                on = ctx.contact_frequencies(s, frames, rings=True)
            r["rows_off"] = int((on["from_ring"] < 0).sum())
            r["ring_rows"] = int((on["from_ring"] >= 0).sum())
            r["rings_on"] = timed(lambda: ctx.contact_frequencies(s, frames, rings=True), 10)
            r["on_over_off"] = round(r["rings_on"]["best_ms"] / r["rings_off"]["best_ms"], 4)
            laps = laps_of(lambda: ctx.contact_frequencies(s, frames, rings=True))
            total = sum(laps.values())
            r["laps_ms"] = {k: round(v, 3) for k, v in laps.items()}
            r["ring_kernels_share"] = round((laps.get("ring fit", 0.0) + laps.get("ring rows", 0.0)) / total, 4) if total else None
            # F = 100: the per-frame loop a user has today
            rec = synth.read_pdb_records(path)
            f100 = frames[:100]
            frame_loop(ctx, rec, f100[:10])  # warm
            loop = timed(lambda: frame_loop(ctx, rec, f100), 3)
            for _ in range(2):
                ctx.contact_frequencies(s, f100, rings=True)
            call = timed(lambda: ctx.contact_frequencies(s, f100, rings=True), 10)
            r["f100"] = {"loop": loop, "call_rings_on": call, "speedup_vs_loop": round(loop["best_ms"] / call["best_ms"], 2)}
        emit(r)
    if not a.off_only:
        rec = synth.gen_stress(n_res=12500, seed=17, box=126.0, hydrogens=False)  # ~10^5 atoms at 0.05 atoms / A^3
        s = aa.Structure.from_records(rec)
        frames = frames_for(s, 20, seed=20)
        r = {"structure": "gen_stress(n_res=12500, box=126)", "frames": 20, "atoms_per_frame": int(frames.shape[1])}
        for _ in range(2):
            ctx.contact_frequencies(s, frames)
            on = ctx.contact_frequencies(s, frames, rings=True)
        r["ring_rows"] = int((on["from_ring"] >= 0).sum())
        r["rings_off"] = timed(lambda: ctx.contact_frequencies(s, frames), 5)
        r["rings_on"] = timed(lambda: ctx.contact_frequencies(s, frames, rings=True), 5)
        r["on_over_off"] = round(r["rings_on"]["best_ms"] / r["rings_off"]["best_ms"], 4)
        laps = laps_of(lambda: ctx.contact_frequencies(s, frames, rings=True))
        total = sum(laps.values())
        r["laps_ms"] = {k: round(v, 3) for k, v in laps.items()}
        r["ring_kernels_share"] = round((laps.get("ring fit", 0.0) + laps.get("ring rows", 0.0)) / total, 4) if total else None
        emit(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
