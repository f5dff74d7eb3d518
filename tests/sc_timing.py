"""Shape complementarity: per-kernel device times (arp_profile_read, summed by name) and the whole call, on 6bft with the reference's
three group sets and on the two-halves interface of tests/test_sc_gpu.py at 10^4 and 10^5 atoms; beside them the single-thread time of
the sequential C restatement (tests/sc_restatement.c) where it is affordable -- labelled as the restatement, not the reference.
Usage: python tests/sc_timing.py"""
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import arpeggia_amd as aa  # noqa: E402
import sc_restatement as R  # noqa: E402
from arpeggia_amd import _lib  # noqa: E402
from test_sc_gpu import two_halves  # noqa: E402


def measure(ctx, name, inp, L=None, reps=3):
    aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"])  # warm-up
    ctx.profile(True)
    acc, wall = {}, []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"])
        wall.append(time.perf_counter() - t0)
        names, ms = (C.c_char_p * 32)(), (C.c_float * 32)()
        k = _lib.lib.arp_profile_read(ctx._h, names, ms, 32)
        for i in range(k):
            acc[names[i].decode()] = acc.get(names[i].decode(), 0.0) + ms[i] / reps
    ctx.profile(False)
    out = {"input": name, "atoms": len(inp["x"]), "sc": res["sc"], "dots": res["combined"]["n_all_dots"], "probes": res["n_probes"],
           "kernels_us": {k: round(v * 1e3, 1) for k, v in acc.items()}, "device_us": round(sum(acc.values()) * 1e3, 1),
           "call_ms_median": round(float(np.median(wall)) * 1e3, 3)}
    if L is not None:
        t0 = time.perf_counter()
        R.run(L, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"])
        out["restatement_cpu_1thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    return out


if __name__ == "__main__":
    ctx = aa.Context(0)
    L = R.compile(tempfile.mkdtemp())
    s = aa.load_model(str(ROOT / "tests" / "data" / "6bft.pdb"))
    for g in ("H/L", "H/C", "H,L/C,G"):
        print(json.dumps(measure(ctx, f"6bft {g}", R.structure_inputs(s, g), L)), flush=True)
    print(json.dumps(measure(ctx, "two halves 1e4", two_halves(10_000), L)), flush=True)
    print(json.dumps(measure(ctx, "two halves 1e5", two_halves(100_000))), flush=True)
