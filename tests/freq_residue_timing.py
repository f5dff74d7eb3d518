"""Timing of residue-level contact frequencies (not a test): python tests/freq_residue_timing.py [--out FILE] [--atom-only] [--label NAME]

1ubq and 6bft x 100 and x 1000 frames (seeded sigma = 0.3 A jitter), rings off and on, every call warm, best / median / minimum / maximum of 10:
  (a) the residue call against the atom-level call on the same input, and -- from the library's `timing` laps of one call, every lap ending in a
      stream synchronise -- where the residue call's time goes ("collapse + reduce" is the lap the residue level adds; the sort is wider);
  (b) for F = 100: the alternative a user has without the feature -- one atomic_contacts call per frame (with rings also one
      Structure.from_records + get_contacts per frame) and a numpy group-by by residue (tests/freq_residue_common.py) -- and the factor;
  (c) --atom-only runs the atom-level calls alone and uses nothing the residue level added: the same file runs against the parent tree's
      package for an A/B in one session; the spread of the 10 repeats stands beside the number.
Prints one JSON line per case.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--atom-only", action="store_true")
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
        all_frames = frames_for(s, 1000, seed=1000)
        for F in (100, 1000):
            frames = all_frames[:F]
            for rings in (False, True):
                r = {"structure": name, "frames": F, "atoms_per_frame": int(frames.shape[1]), "rings": rings}
                atom = lambda: ctx.contact_frequencies(s, frames, rings=rings)
                for _ in range(2):
                    t = atom()  # warm: workspace, buffers
                r["atom_rows"] = int(len(t["n_frames"]))
                r["atom"] = timed(atom, 10)
                if not a.atom_only:
                    import freq_residue_common as fc

                    res = lambda: ctx.contact_frequencies(s, frames, rings=rings, level="residue")
                    for _ in range(2):
                        t = res()
                    r["residue_rows"] = int(len(t["n_frames"]))
                    r["residue"] = timed(res, 10)
                    r["residue_over_atom"] = round(r["residue"]["best_ms"] / r["atom"]["best_ms"], 4)
                    r["laps_atom_ms"] = {k: round(v, 3) for k, v in laps_of(atom).items()}
                    r["laps_residue_ms"] = {k: round(v, 3) for k, v in laps_of(res).items()}
                    if F == 100:  # the per-frame loop a user has today, grouped by residue in numpy
                        rec = synth.read_pdb_records(path) if rings else None
                        loop = lambda: fc.expected(ctx, s, frames, "/", rec=rec)
                        fc.expected(ctx, s, frames[:10], "/", rec=rec)  # warm
                        r["loop"] = timed(loop, 3)
                        r["speedup_vs_loop"] = round(r["loop"]["best_ms"] / r["residue"]["best_ms"], 2)
                emit(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
