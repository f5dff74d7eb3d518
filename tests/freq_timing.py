"""Timing of arp_contact_frequencies (not a test): python tests/freq_timing.py [--out FILE] [--quick]

For 1ubq x {100, 1000, 10 000} and 6bft x {100, 1000} frames (seeded sigma = 0.3 A jitter): the call (warm; best and median of the repeats) and
the time per frame; the baseline of one atomic_contacts call per frame + numpy aggregation; and, for F <= 100, get_contacts on the
multi-model file of the same frames + a group-by.  Prints one JSON line per case.
"""
from __future__ import annotations

import argparse
import json
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
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, float(np.median(ts)) * 1e3


def loop_baseline(ctx, s, frames):
    """One atomic_contacts call per frame (contacts only), then (i, j, code) -> count / min / max in numpy."""
    soa = s.soa("/")
    n = frames.shape[1]
    top = {k: soa[k][:n] for k in ("attr", "res_ord", "chain_rank", "model", "res_id", "res_cb", "res_sg", "res_h_ptr", "res_h_idx")}
    prm = aa.default_params(contacts_only=True)
    keys, dists = [], []
    for f in range(frames.shape[0]):
        p = ctx.atomic_contacts(dict(top, x=frames[f, :, 0], y=frames[f, :, 1], z=frames[f, :, 2]), prm)
        kind = p["kind"]
        for code in np.flatnonzero(np.bitwise_or.reduce(kind) >> np.arange(19) & 1) if len(kind) else []:
            sel = (kind >> np.uint32(code)) & np.uint32(1) == 1
            keys.append((p["i"][sel].astype(np.uint64) << np.uint64(34)) | (p["j"][sel].astype(np.uint64) << np.uint64(5)) | np.uint64(code))
            dists.append(p["dist"][sel])
    k = np.concatenate(keys)
    d = np.concatenate(dists)
    uk, inv, cnt = np.unique(k, return_inverse=True, return_counts=True)
    mn = np.full(len(uk), np.inf, np.float32); np.minimum.at(mn, inv, d)
    mx = np.full(len(uk), -np.inf, np.float32); np.maximum.at(mx, inv, d)
    return len(uk)


def model_file_baseline(ctx, path, n):
    s = aa.load_model(str(path))
    t = ctx.get_contacts(s, "/", 0.1, 6.5)
    a = (t["from_atom"] >= 0) & (t["to_atom"] >= 0)
    key = ((t["from_atom"][a] % n).astype(np.uint64) << np.uint64(34)) | ((t["to_atom"][a] % n).astype(np.uint64) << np.uint64(5)) | t["interaction"][a].astype(np.uint64)
    return len(np.unique(key))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--profile", action="store_true", help="only the calls (1ubq x 1000, 6bft x 1000, 5 each): the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    ctx = aa.Context(0)
    if a.profile:
        for name in ("1ubq", "6bft"):
            s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
            frames = frames_for(s, 1000, seed=1000)
            for _ in range(5):
                ctx.contact_frequencies(s, frames)
        return
    cases = [("1ubq", 100), ("1ubq", 1000), ("1ubq", 10000), ("6bft", 100), ("6bft", 1000)]
    if a.quick:
        cases = [("1ubq", 100), ("1ubq", 1000)]
    lines = []
    for name, F in cases:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        frames = frames_for(s, F, seed=F)
        n = frames.shape[1]
        reps = 10 if F <= 1000 else 3
        ctx.contact_frequencies(s, frames)  # warm: workspace, buffers
        rows = len(ctx.contact_frequencies(s, frames)["n_frames"])
        best, med = timed(lambda: ctx.contact_frequencies(s, frames), reps)
        loop_reps = 3 if F <= 1000 else 1
        loop_baseline(ctx, s, frames[: min(F, 50)])  # warm
        lb, lm = timed(lambda: loop_baseline(ctx, s, frames), loop_reps)
        r = {"structure": name, "frames": F, "atoms_per_frame": n, "rows": rows, "call_best_ms": round(best, 3), "call_median_ms": round(med, 3),
             "us_per_frame": round(best * 1e3 / F, 3), "loop_best_ms": round(lb, 3), "loop_median_ms": round(lm, 3),
             "loop_us_per_frame": round(lb * 1e3 / F, 3), "speedup_vs_loop": round(lb / best, 2)}
        if F <= 100:
            rec = synth.read_pdb_records(ROOT / "tests" / "data" / f"{name}.pdb")
            with tempfile.TemporaryDirectory() as td:
                # the frames as MODEL records (3 decimals, as PDB stores them); the topology's atoms only (load_model's filter)
                top = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
                serial = top.ints("atomi")
                sel = np.searchsorted(rec["serial"], serial)
                parts = []
                for m in range(F):
                    r_ = {k: v[sel].copy() for k, v in rec.items()}
                    r_["x"], r_["y"], r_["z"] = (np.round(frames[m, :, c], 3) for c in range(3))
                    r_["model_serial"][:] = m + 1
                    parts.append(r_)
                path = Path(td) / "models.pdb"
                synth.write_pdb({k: np.concatenate([p[k] for p in parts]) for k in rec}, path)
                model_file_baseline(ctx, path, n)
                mb, mm = timed(lambda: model_file_baseline(ctx, path, n), 3)
                sm = aa.load_model(str(path))
                fb, fm = timed(lambda: ctx.contact_frequencies(sm, None), 5)
            r.update(model_file_get_contacts_best_ms=round(mb, 3), model_file_get_contacts_median_ms=round(mm, 3),
                     model_file_freq_best_ms=round(fb, 3))
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
