"""Timing of the secondary-structure call (not a test): python tests/dssp_timing.py [--out FILE] [--reps N] [--cases 1ubq:1000,...] [--no-host]

1ubq x 1000 and x 10 000 frames, 6bft x 100 and x 1000 frames: the file's atoms with a seeded 0.3 A jitter per atom and frame.  Warm (two calls first), then
--reps calls (default 5), best / median / max:
  call          Context.secondary_structure(codes=True, hbonds=False) from the frames in host memory to the result in host memory
  laps_ms       the library's `timing` laps of one call, added up over the upload passes: upload, pack (k_dssp_pack), sweep (k_dssp_sweep), assign
                (k_dssp_assign), download; and each one's share of their sum
  sweep         from the shapes: F R^2 (acceptor, donor) pairs; every pair costs at least the CA test -- 3 subtractions, 3 multiplications, 2 additions in f64,
                no FMA (the library is built with -ffp-contract=off) -- so the least time the vector units could take is pairs x 8 instructions over the f64
                vector instruction rate.  MI355X_MICROARCH.md lists no f64 vector figure; the rate used is the datasheet's 78.6 TFLOP/s (spec, FMA = 2) / 2.
                pairs_per_s, bound_ms and share_of_bound = bound_ms / the sweep lap
  host          arp_dssp_host over the same frames, gathered by backbone_select, split over 16 processes (spawned, no device), wall time of the pool's map with
                the workers already started; and whether every output equals the device's
Prints one JSON line per case.
"""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
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

F64_VECTOR_TFLOPS_SPEC = 78.6   # MI355X datasheet, FMA counted as 2
CA_TEST_INSTRUCTIONS = 8
HOST_PROCESSES = 16


def host_part(args):
    import arpeggia_amd as aa

    bb_xyz, flags = args
    return aa.secondary_structure_host(bb_xyz, flags, codes=True, hbonds=False)


def warm(_):
    import arpeggia_amd  # noqa: F401

    return os.getpid()


def laps_of(aa, fn) -> dict:
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
        m = re.match(r"\s*dssp (\S+)\s+([0-9.]+) ms", line)
        if m:
            laps[m.group(1)] = round(laps.get(m.group(1), 0.0) + float(m.group(2)), 3)
    return laps


def timed(fn, reps: int) -> dict:
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # (the call ends in a download: the device has drained)
        t.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(t), 3), "median_ms": round(float(np.median(t)), 3), "max_ms": round(max(t), 3), "repeats": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=5, type=int)
    ap.add_argument("--cases", default="1ubq:1000,1ubq:10000,6bft:100,6bft:1000")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (when comparing builds of the sweep)")
    a = ap.parse_args()
    pool = mp.get_context("spawn").Pool(HOST_PROCESSES)   # started before the device is opened; the workers never open it
    pool.map(warm, range(HOST_PROCESSES * 4))
    import arpeggia_amd as aa
    import trajectory_shapes as ts

    ctx = aa.Context(0)
    lines = []
    for name, F in [(c.split(":")[0], int(c.split(":")[1])) for c in a.cases.split(",")]:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        n = aa.api._topology_atoms(s)
        soa = s.soa("/")
        base = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
        frames = ts.jitter(base, F, seed=F)
        sel = aa.backbone_select(s)
        R = int(len(sel["atom"]))
        call = lambda: ctx.secondary_structure(s, frames, codes=True, hbonds=False)
        for _ in range(2):
            got = call()
        r = {"structure": name, "frames": F, "residues": R, "atoms_per_frame": n, "call": timed(call, a.reps), "laps_ms": laps_of(aa, call)}
        total = sum(r["laps_ms"].values())
        r["lap_share"] = {k: round(v / total, 4) for k, v in r["laps_ms"].items()} if total else {}
        pairs = F * R * R
        bound_ms = pairs * CA_TEST_INSTRUCTIONS / (F64_VECTOR_TFLOPS_SPEC * 1e12 / 2.0) * 1e3
        sweep_ms = r["laps_ms"].get("sweep")
        r["sweep"] = {"pairs": pairs, "bound_ms": round(bound_ms, 4), "f64_vector_tflops_spec": F64_VECTOR_TFLOPS_SPEC, "instructions_per_pair_at_least": CA_TEST_INSTRUCTIONS}
        if sweep_ms:
            r["sweep"].update({"lap_ms": sweep_ms, "pairs_per_s": round(pairs / (sweep_ms * 1e-3), 1), "share_of_bound": round(bound_ms / sweep_ms, 4)})
        if a.no_host:
            print(json.dumps(r), flush=True)
            lines.append(r)
            continue
        bbx = frames[:, sel["bb"]]
        parts = [(bbx[k::HOST_PROCESSES], sel["flags"]) for k in range(HOST_PROCESSES) if len(bbx[k::HOST_PROCESSES])]
        t, host = [], None
        for _ in range(max(2, a.reps // 2)):
            t0 = time.perf_counter()
            host = pool.map(host_part, parts)
            t.append((time.perf_counter() - t0) * 1e3)
        r["host"] = {"processes": len(parts), "best_ms": round(min(t), 3), "median_ms": round(float(np.median(t)), 3), "max_ms": round(max(t), 3), "repeats": len(t)}
        codes = np.zeros_like(got["codes"])
        for k, part in enumerate(host):
            codes[k::HOST_PROCESSES] = part["codes"]
        r["equal_to_host"] = bool(np.array_equal(codes, got["codes"]) and np.array_equal(sum(p["counts"] for p in host), got["counts"]))
        r["speedup_vs_host"] = round(r["host"]["best_ms"] / r["call"]["best_ms"], 2)
        r["spreads_apart"] = r["call"]["max_ms"] < r["host"]["best_ms"]
        print(json.dumps(r), flush=True)
        lines.append(r)
    pool.close()
    pool.join()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
