"""Timing of water bridges (not a test): python tests/water_bridge_timing.py [--out FILE] [--flag-off] [--label NAME] [--package-root DIR]

Every call warm, best / median / minimum / maximum of 10 (5 for the largest solvated case):
  (a) waters on against off for the residue frequency call and the residue timeline call on 1ubq x 1000 frames (seeded sigma = 0.3 A jitter) and on a
      synthetic solvated case -- 1ubq plus 10^3, 10^4 and 3 x 10^4 waters at bulk density (0.0334 per A^3, a cube around the protein, none within
      2.4 A of a protein atom) x 20 frames -- with the water kernel's share of the frequency call from the library's `timing` laps (every lap ends in
      a stream synchronise);
  (b) arp_water_bridges on 1ubq x 1000 frames against the numpy restatement (tests/water_bridge_restatement.py) run frame by frame in 16 processes;
  (c) --flag-off runs the flag-off calls of (a) on 1ubq x 1000 frames alone and uses nothing this feature added, so the same file runs against the
      parent tree's package (--package-root) for an interleaved A/B; the spread of the repeats stands beside the number.
Prints one JSON line per case."""
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
UBQ = ROOT / "tests" / "data" / "1ubq.pdb"
BULK = 0.0334  # waters per cubic angstrom


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # (every call ends in the download of its table: the device has drained)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "repeats": reps}


def laps_of(aa, fn) -> dict:
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


def jitter(base, F, seed):
    return base[None] + np.random.default_rng(seed).normal(scale=0.3, size=(F,) + base.shape)


def solvated(rec: dict, n_water: int, seed: int) -> dict:
    """The records of 1ubq without its own waters, plus n_water waters (chain W) uniformly in a cube of n_water / BULK cubic angstrom around the protein."""
    keep = rec["resn"] != b"HOH"
    rec = {k: v[keep] for k, v in rec.items()}
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    side = (n_water / BULK) ** (1.0 / 3.0)
    rng = np.random.default_rng(seed)
    pts = np.zeros((0, 3))
    while len(pts) < n_water:
        cand = xyz.mean(0) + rng.uniform(-side / 2, side / 2, (2 * n_water, 3))
        far = np.ones(len(cand), bool)
        for k0 in range(0, len(cand), 4096):
            d = cand[k0:k0 + 4096, None, :] - xyz[None]
            far[k0:k0 + 4096] = ((d * d).sum(2) > 2.4 * 2.4).all(1)
        pts = np.concatenate([pts, cand[far]])[:n_water]
    w = {"x": pts[:, 0], "y": pts[:, 1], "z": pts[:, 2], "occupancy": np.ones(n_water), "serial": 100000 + np.arange(n_water), "resi": 1 + np.arange(n_water),
         "name": np.full(n_water, b"O", "S8"), "resn": np.full(n_water, b"HOH", "S8"), "chain": np.full(n_water, b"W", "S8"), "altloc": np.full(n_water, b"", "S4"),
         "icode": np.full(n_water, b"", "S4"), "element": np.full(n_water, b"O", "S4"), "model_serial": np.zeros(n_water)}
    return {k: np.concatenate([rec[k], np.asarray(w[k]).astype(rec[k].dtype)]) for k in rec}


_WORKER = {}


def _worker_init(root: str):
    for p in (root, str(Path(root) / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import arpeggia_amd as aa
    import water_bridge_restatement as wr

    s = aa.load_model(str(UBQ))
    _WORKER.update(wr=wr, cls=wr.classify(s, s.n_atoms, "/"), s=s)


def _worker_frames(job):
    f0, frames = job
    wr, (soa, water, polar) = _WORKER["wr"], _WORKER["cls"]
    return sum(len(wr.frame_triples(soa, water, polar, frames[k], f0 + k)) for k in range(len(frames)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--flag-off", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--package-root", default=str(ROOT))
    ap.add_argument("--reps", default=10, type=int)
    a = ap.parse_args()
    for p in (a.package_root, str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import arpeggia_amd as aa

    s = aa.load_model(str(UBQ))
    soa = s.soa("/")
    base = np.stack([soa["x"], soa["y"], soa["z"]], 1)
    frames = jitter(base, 1000, seed=3000)
    restatement = None
    if not a.flag_off:  # (b)'s host side first: the worker processes start and end before this process opens the device
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor

        with ProcessPoolExecutor(16, mp_context=mp.get_context("spawn"), initializer=_worker_init, initargs=(str(ROOT),)) as pool:
            jobs = [(f0, frames[f0:f0 + 10]) for f0 in range(0, 1000, 10)]
            list(pool.map(_worker_frames, jobs[:16]))  # warm: the workers are up
            t0 = time.perf_counter()
            total = sum(pool.map(_worker_frames, jobs))
            restatement = (total, round((time.perf_counter() - t0) * 1e3, 1))
    ctx = aa.Context(0)
    lines = []

    def emit(r):
        if a.label:
            r = dict(label=a.label, **r)
        print(json.dumps(r), flush=True)
        lines.append(r)

    def on_off(name, s, frames, reps, waters=(False, True)):
        r = {"case": name, "frames": int(frames.shape[0]), "atoms_per_frame": int(frames.shape[1])}
        for what, call in (("frequency", ctx.contact_frequencies), ("timeline", ctx.contact_timelines)):
            for w in waters:
                fn = (lambda: call(s, frames, level="residue", waters=True)) if w else (lambda: call(s, frames, level="residue"))
                for _ in range(2):
                    t = fn()  # warm: workspace, buffers
                key = f"{what}_{'on' if w else 'off'}"
                r[key] = timed(fn, reps)
                r[key + "_rows"] = int(len(t["n_frames"]))
                if w:
                    r[what + "_water_rows"] = int((t["interaction"] == 19).sum())
                    if what == "frequency":
                        laps = laps_of(aa, fn)
                        r["laps_on_ms"] = {k: round(v, 3) for k, v in laps.items()}
                        r["water_kernel_share_of_laps"] = round(laps.get("water bridges", 0.0) / max(sum(laps.values()), 1e-9), 4)
            if len(waters) == 2:
                r[what + "_on_over_off"] = round(r[what + "_on"]["best_ms"] / r[what + "_off"]["best_ms"], 4)
        emit(r)

    if a.flag_off:
        on_off("1ubq", s, frames, a.reps, waters=(False,))
    else:
        import synth

        on_off("1ubq", s, frames, a.reps)
        # (b) the triples against the restatement, frame by frame in 16 processes
        call = lambda: ctx.water_bridges(s, frames, "/")
        for _ in range(2):
            t = call()
        r = {"case": "1ubq water_bridges", "frames": 1000, "rows": int(len(t["frame"])), "device": timed(call, a.reps)}
        r["restatement_16_processes_ms"] = restatement[1]
        assert restatement[0] == r["rows"], (restatement[0], r["rows"])
        r["speedup"] = round(r["restatement_16_processes_ms"] / r["device"]["best_ms"], 1)
        emit(r)
        rec = synth.read_pdb_records(UBQ)
        for n_water in (1000, 10000, 30000):
            sol = solvated(rec, n_water, seed=n_water)
            ss = aa.Structure.from_records(sol)
            b = np.stack([sol["x"], sol["y"], sol["z"]], 1)
            on_off(f"1ubq + {n_water} waters", ss, jitter(b, 20, seed=20 + n_water), 5 if n_water >= 30000 else a.reps)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
