"""Timing of the RMSF call (not a test): python tests/rmsf_timing.py [--out FILE] [--reps N] [--cases 1ubq:ca:ca:1000,...]

1ubq CA x 1000 and x 10 000 frames, 1ubq fit CA / measure heavy x 10 000, 6bft CA x 1000, on the frames of tests/rmsd_timing.py (40 states + a 0.3 A jitter,
tumbled and shifted), each with reference="mean" (iterated from frame 0, the Python layer's default max_rounds and tol) and with the fixed reference frame 0.
Warm (two calls first), best of --reps (default 5) calls of Context.rmsf, without the optional outputs:
  device       the call, and from the library's `timing` laps of one call its split: pack (upload + k_rmsd_pack) / fit (k_rmsf_fit) / sweep (k_rmsf_sweep,
               the mean) / finish (k_rmsf_mean_finish + k_rmsf_change + the 8-byte read-back), summed over the rounds / deviation / download
  bytes        what each kernel of a round reads and writes, from the shapes, and the rate that gives over its lap divided by the rounds
  numpy_route  the reference of tests/rmsf_cases.py -- centre, batched einsum, batched SVD, rotate, mean, the same rounds -- on the host's threads, best of 2;
               its result is compared with the call's (rounds, largest error / bound)
  rmsd         Context.rmsd to frame 0 on the same frames, for scale
Prints one JSON line per case and reference kind.
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
import rmsf_cases as fc  # noqa: E402
from rmsd_timing import frames_for, timed  # noqa: E402


def laps_of(fn) -> dict:
    """The `timing` laps one call prints on stderr: {lap: ms}, laps of the same name (one per round) added up."""
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
        m = re.match(r"\s*rmsf (\S+)\s+([0-9.]+) ms", line)
        if m:
            laps[m.group(1)] = round(laps.get(m.group(1), 0.0) + float(m.group(2)), 3)
    return laps


def round_bytes(F: int, n: int) -> dict:
    """Bytes one round's kernels move, from the shapes (n_pad: n rounded up to 4; 32 frames per slab)."""
    n_pad, slabs = -(-n // 4) * 4, -(-F // fc.SLAB)
    x = F * 3 * n_pad * 8
    return {"fit": x + 3 * n_pad * 8 + F * 72, "sweep": x + F * 72 + slabs * 3 * n_pad * 8, "finish": slabs * 3 * n_pad * 8 + 2 * 3 * n_pad * 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=5, type=int)
    ap.add_argument("--cases", default="1ubq:ca:ca:1000,1ubq:ca:ca:10000,1ubq:ca:heavy:10000,6bft:ca:ca:1000")
    a = ap.parse_args()
    ctx = aa.Context(0)
    lines = []
    for name, fit, atoms, F in [(c.split(":")[0], c.split(":")[1], c.split(":")[2], int(c.split(":")[3])) for c in a.cases.split(",")]:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        sel = aa.rmsd_select(s, fit)
        msel = None if atoms == fit else aa.rmsd_select(s, atoms)
        frames = frames_for(s, F, seed=F)
        X, XM = frames[:, sel], None if msel is None else frames[:, msel]
        rmsd_call = lambda: ctx.rmsd(s, frames, reference=0, atoms=sel)
        for _ in range(2):
            rmsd_call()
        rmsd_time = timed(rmsd_call, a.reps)
        for reference in ("mean", 0):
            call = lambda: ctx.rmsf(s, frames, fit=sel, atoms=msel, reference=reference)
            for _ in range(2):
                got = call()
            r = {"structure": name, "fit": fit, "atoms": atoms, "n": int(len(sel)), "m": int(len(sel) if msel is None else len(msel)), "frames": F,
                 "atoms_per_frame": int(frames.shape[1]), "reference": reference, "rounds": got["n_rounds"], "last_change": got["last_change"], "converged": got["converged"],
                 "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()}
            r["device"] = timed(call, a.reps)
            r["device"]["laps_ms"] = laps = laps_of(call)
            r["round_bytes"] = round_bytes(F, len(sel))
            r["round_gb_per_s"] = {k: round(b * got["n_rounds"] / (laps[k] * 1e-3) / 1e9, 1) for k, b in r["round_bytes"].items() if laps.get(k)}
            kw = dict(ref=0, max_rounds=50 if reference == "mean" else 1, tol=1e-4 if reference == "mean" else 0.0)
            t = []
            for _ in range(2):
                t0 = time.perf_counter()
                ref = fc.reference(X, XM, **kw)
                t.append((time.perf_counter() - t0) * 1e3)
            r["numpy_route"] = {"best_ms": round(min(t), 1), "rounds": ref["n_rounds"], "repeats": 2}
            r["speedup_vs_numpy_route"] = round(min(t) / r["device"]["best_ms"], 2)
            r["error_over_bound"] = round(fc.assert_within(got, ref, (name, fit, atoms, F, reference)), 4) if ref["n_rounds"] == got["n_rounds"] else "rounds differ"
            r["rmsd_to_frame_0"] = rmsd_time
            r["time_over_rmsd"] = round(r["device"]["best_ms"] / rmsd_time["best_ms"], 2)
            print(json.dumps(r), flush=True)
            lines.append(r)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
