"""Timing of the covariance, DCCM, PCA and projection calls (not a test): python tests/cov_timing.py [--out FILE] [--reps N] [--cases 1ubq:ca:ca:1000,...]

1ubq CA x 1000 and x 10 000 frames, 1ubq fit CA / measure heavy x 10 000, 6bft CA x 1000, on the frames of tests/rmsd_timing.py, reference="mean" (the Python
layer's default max_rounds and tol).  Warm (two calls first), best of --reps (default 5):
  covariance, dccm   Context.covariance with the one output, and from the library's `timing` laps of one call the split behind arp_rmsf's own laps:
                     cov_dev (k_cov_dev) / cov_gram, dccm_gram (k_cov_gram) / cov_finish, dccm_finish (the finish kernels and the download of the matrix)
  gram               from the shapes: the MFMA flops the Gram kernel issues (whole 32 x 32 tiles of the upper triangle) and the useful ones (L^2 F), the bytes
                     it reads (two operand panels per tile and slab) and writes (the slab partials), and the rates those give over its lap
  pca                Context.pca(n_modes=10), and the share of it spent in numpy.linalg.eigh (pca_modes on the call's own covariance, timed alone)
  project            Context.project of the same frames onto the ten modes
  parent_route       what a user had before this call: Context.rmsf(aligned=True), then numpy D^T D / F on the host's threads (and, for the dccm, the reduction
                     of its 3 x 3 blocks' traces and the normalisation)
  numpy_route        the reference of tests/cov_cases.py without its bounds: rmsf_cases.reference, D^T D / F and the dccm formula; best of 2; its result is
                     compared with the call's (largest error / bound, cov_cases' bounds computed once)
  rmsf               Context.rmsf on the same frames without the optional outputs, for scale
Prints one JSON line per case.
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
import cov_cases as cc  # noqa: E402
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


def gram_work(F: int, L: int, rows_per_frame: int) -> dict:
    """Flops and bytes of one k_cov_gram launch over L rows and columns (cov: L = 3 m_pad, one contraction row per frame; dccm: L = m_pad, three)."""
    slab, slabs = cc.slab_plan(F, L)
    T = -(-L // cc.TILE)
    tri = T * (T + 1) // 2
    K = F * rows_per_frame
    return {"tiles": tri, "slab_frames": slab, "slabs": slabs, "workgroups": tri * slabs, "mfma_flops": 2 * tri * cc.TILE * cc.TILE * K, "useful_flops": L * L * K,
            "read_bytes": tri * 2 * cc.TILE * K * 8, "partial_bytes": tri * slabs * cc.TILE * cc.TILE * 8, "operand_bytes": K * L * 8}


def best_of(fn, reps: int) -> tuple:
    t, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(t), 3), "median_ms": round(float(np.median(t)), 3), "max_ms": round(max(t), 3), "repeats": reps}, out


def dccm_from_cov(cov: np.ndarray) -> np.ndarray:
    m = len(cov) // 3
    return cc.dccm_of(cov.reshape(m, 3, m, 3)[:, [0, 1, 2], :, [0, 1, 2]].sum(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=5, type=int)
    ap.add_argument("--cases", default="1ubq:ca:ca:1000,1ubq:ca:ca:10000,1ubq:ca:heavy:10000,6bft:ca:ca:1000")
    ap.add_argument("--no-bounds", action="store_true", help="skip the error / bound comparison (the bounds cost several host products of the cov's size)")
    a = ap.parse_args()
    ctx = aa.Context(0)
    lines = []
    for name, fit, atoms, F in [(c.split(":")[0], c.split(":")[1], c.split(":")[2], int(c.split(":")[3])) for c in a.cases.split(",")]:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        sel = aa.rmsd_select(s, fit)
        msel = None if atoms == fit else aa.rmsd_select(s, atoms)
        idx = sel if msel is None else msel
        m = int(len(idx))
        frames = frames_for(s, F, seed=F)
        X, XM = frames[:, sel], None if msel is None else frames[:, msel]
        r = {"structure": name, "fit": fit, "atoms": atoms, "n": int(len(sel)), "m": m, "frames": F, "atoms_per_frame": int(frames.shape[1]), "reference": "mean",
             "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()}
        calls = {"rmsf": lambda: ctx.rmsf(s, frames, fit=sel, atoms=msel), "covariance": lambda: ctx.covariance(s, frames, fit=sel, atoms=msel, cov=True, dccm=False),
                 "dccm": lambda: ctx.dccm(s, frames, fit=sel, atoms=msel), "pca": lambda: ctx.pca(s, frames, fit=sel, atoms=msel, n_modes=10)}
        got = {}
        for key, fn in calls.items():
            for _ in range(2):
                got[key] = fn()
            r[key] = timed(fn, a.reps)
            if key in ("covariance", "dccm"):
                r[key]["laps_ms"] = laps_of(fn)
        r["rounds"], r["converged"] = got["covariance"]["n_rounds"], got["covariance"]["converged"]
        m_pad = cc.pad(m)
        for key, lap, work in (("covariance", "cov_gram", gram_work(F, 3 * m_pad, 1)), ("dccm", "dccm_gram", gram_work(F, m_pad, 3))):
            ms = r[key]["laps_ms"].get(lap)
            if ms:
                work["lap_ms"] = ms
                work["mfma_tflops"], work["useful_tflops"] = round(work["mfma_flops"] / (ms * 1e-3) / 1e12, 3), round(work["useful_flops"] / (ms * 1e-3) / 1e12, 3)
                work["read_gb_per_s"] = round(work["read_bytes"] / (ms * 1e-3) / 1e9, 1)
            r[lap] = work
        pca = got["pca"]
        r["eigh"] = timed(lambda: aa.pca_modes(pca["covariance"], 10), a.reps)
        r["eigh_share_of_pca"] = round(r["eigh"]["best_ms"] / r["pca"]["best_ms"], 3)
        project = lambda: ctx.project(s, frames, idx, pca["mean"], pca["modes"], pca["transforms"])
        for _ in range(2):
            project()
        r["project"] = timed(project, a.reps)

        def parent_cov():
            rm = ctx.rmsf(s, frames, fit=sel, atoms=msel, aligned=True)
            D = (rm["aligned"] - rm["mean"]).reshape(F, -1)
            return D.T @ D / F

        r["parent_route_covariance"], pc = best_of(parent_cov, a.reps)
        r["parent_route_dccm"], pd = best_of(lambda: dccm_from_cov(parent_cov()), a.reps)
        r["rmsf_aligned"] = timed(lambda: ctx.rmsf(s, frames, fit=sel, atoms=msel, aligned=True), a.reps)
        r["speedup_vs_parent_route"] = {"covariance": round(r["parent_route_covariance"]["best_ms"] / r["covariance"]["best_ms"], 2),
                                        "dccm": round(r["parent_route_dccm"]["best_ms"] / r["dccm"]["best_ms"], 2)}
        r["spreads_apart"] = {"covariance": r["covariance"]["max_ms"] < r["parent_route_covariance"]["best_ms"], "dccm": r["dccm"]["max_ms"] < r["parent_route_dccm"]["best_ms"]}

        def numpy_route():
            base = fc.reference(X, XM, 0, 50, 1e-4)
            D = cc.deviations(base)
            cov = D.T @ D / F
            return base, cov, dccm_from_cov(cov)

        r["numpy_route"], (base, ncov, ndccm) = best_of(numpy_route, 2)
        r["speedup_vs_numpy_route"] = {"covariance": round(r["numpy_route"]["best_ms"] / r["covariance"]["best_ms"], 2), "dccm": round(r["numpy_route"]["best_ms"] / r["dccm"]["best_ms"], 2)}
        r["largest_difference_to_parent_route"] = {"covariance": float(np.abs(pc - got["covariance"]["covariance"]).max()), "dccm": float(np.abs(pd - got["dccm"]["dccm"]).max())}
        if base["n_rounds"] != r["rounds"]:
            r["error_over_bound"] = "rounds differ"
        elif not a.no_bounds:
            ref = dict(cc.second_moments(cc.deviations(base), cc.tau_of(base)), base=base)
            r["error_over_bound"] = {"covariance": round(cc.assert_within(got["covariance"], ref, name, keys=("covariance",)), 4),
                                     "dccm": round(cc.assert_within(got["dccm"], ref, name, keys=("dccm",)), 4)}
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
