"""Atom SASA (include/arpeggia_amd.h "atom SASA"): device time of the grid build and of the Shrake-Rupley kernel, the call time, and the
number of f32 distance tests the kernel made, on 1ubq, 6bft and S1 clouds, for 100 sphere points.  The work is VALU-bound: each test is
~10 vector instructions (3 adds, 2 FMAs, 1 multiply, 2 compares, the ballot bookkeeping), so the report gives the FP32 FLOP rate those tests
imply (6 FLOP per test: 3 adds + 2 FMAs counted as 2 each, the multiply not counted) as a share of the MI355X vector peak, 157.3 TFLOPS.
Usage: python tests/sasa_timing.py [atoms ...]   (S1 sizes; default 100000 1000000)"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import arpeggia_amd as aa  # noqa: E402
import synth  # noqa: E402
from arpeggia_amd import _lib  # noqa: E402

PEAK_FP32_TFLOPS = 157.3  # MI355X vector FP32 peak (MI355X_MICROARCH guide)
FLOP_PER_TEST = 6


def radii(elements):
    p = aa.default_params()
    return np.array([p.vdw_radius[_lib.lib.arp_element_class(e)] for e in elements], dtype=np.float32)


def measure(ctx, name, x, y, z, r, reps=5, n_points=100):
    aa.atom_sasa(ctx, x, y, z, r, n_points=n_points)  # warm-up (workspace, scratch)
    ctx.profile(True)
    acc, wall = {}, []
    for _ in range(reps):
        t0 = time.perf_counter()
        sasa, _ = aa.atom_sasa(ctx, x, y, z, r, n_points=n_points)
        wall.append(time.perf_counter() - t0)
        for k, v in ctx.profile_read().items():
            acc[k] = acc.get(k, 0.0) + v / reps
    ctx.profile(False)
    tests = aa.sasa_tests(ctx)
    k_ms = acc.get("sasa", 0.0)
    return {"input": name, "atoms": len(x), "n_points": n_points, "kernels_us": {k: round(v * 1e3, 1) for k, v in acc.items()},
            "sasa_kernel_us": round(k_ms * 1e3, 1), "device_us_per_call": round(sum(acc.values()) * 1e3, 1),
            "call_ms_median": round(float(np.median(wall)) * 1e3, 3), "distance_tests": int(tests),
            "tests_per_atom_point": round(tests / (len(x) * n_points), 2),
            "fp32_share_of_peak": (tests * FLOP_PER_TEST / (k_ms * 1e-3)) / (PEAK_FP32_TFLOPS * 1e12) if k_ms else None,
            "total_sasa": float(sasa.astype(np.float64).sum())}


if __name__ == "__main__":
    ctx = aa.Context(0)
    for f in ("1ubq", "6bft"):
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{f}.pdb"))
        sel = aa.sasa_select(s)
        soa = s.soa()
        print(json.dumps(measure(ctx, f, soa["x"][sel], soa["y"][sel], soa["z"][sel], radii(s.strings("element")[sel]))), flush=True)
    for a in [int(v) for v in sys.argv[1:]] or [100_000, 1_000_000]:
        rec = synth.gen_s1(a)
        print(json.dumps(measure(ctx, f"S1 {a}", rec["x"], rec["y"], rec["z"], radii(rec["element"]))), flush=True)
