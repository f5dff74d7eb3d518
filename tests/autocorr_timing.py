"""Timing of contact autocorrelation (not a test): python tests/autocorr_timing.py [--out FILE] [--reps N] [--label NAME] [--cases 1ubq:1000,...] [--no-host]

1ubq x 1000, 1ubq x 10 000 and 6bft x 1000 frames (seeded sigma = 0.3 A jitter), atom and residue level, both modes, L = F - 1 and L = 100.  Warm, best of
--reps (default 5) calls:
  autocorrelation  Context.contact_autocorrelation
  timelines        Context.contact_timelines(bitmap=False) on the same arguments: the floor, the two sweeps the call shares
From the library's `timing` laps of one call: the split rows / marks / curves / download and the kernels alone from device events, with the rate in useful
word-lags per second (intermittent: rows x the sum over the lags of W - lag // 32 words) and its share of the vector ceiling of DESIGN.md section 3.14
(7.9e13 lane operations per second) at the kernel's three vector instructions per word-lag (funnel shift, AND, popcount-accumulate).
Beside it, once per input, level and mode, what a user has without the call, on the bitmap of contact_timelines(bitmap=True).  Every host route runs
on 16 threads, each with its own block of rows (on_row_blocks; the thread variables of numpy's libraries are set to 16 before numpy is imported), and is
checked for counts identical to the call's:
  numpy_per_lag    (m[:, :F - t] & m[:, t:]).sum(1) lag by lag (continuous: the iterated AND); all lags when that takes under about 10 s, else 32 evenly
                   spaced lags (intermittent) or the first 32 (continuous) and the per-lag cost times the lag count, marked "extrapolated"
  fast_host        the fastest exact host route written with numpy alone: intermittent -- rfft autocorrelation of the rows in f64, rounded to integers;
                   continuous -- a run-length histogram per row and two suffix sums
added_to_floor_ms is the call's best minus the floor's best, floor_spread_ms the floor's max minus best of its repeats; the ratios of the host routes to
what the call adds are recorded only where that difference is more than twice the spread.  Prints one JSON line per case.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HOST_THREADS = 16
for _var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # before numpy loads its libraries
    os.environ.setdefault(_var, str(HOST_THREADS))

import numpy as np  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT / "tests"), str(ROOT)):
    if p in sys.path:
        sys.path.remove(p)
    sys.path.insert(0, p)

import arpeggia_amd as aa  # noqa: E402

CEILING_LANE_OPS = 7.9e13   # 256 CUs x 4 SIMDs x 32 lanes per cycle at 2.4 GHz
INSTR_PER_WORD_LAG = 3      # v_alignbit_b32, v_and_b32, v_bcnt_u32_b32 (the LDS read of the shifted word is not a vector-ALU instruction)


def frames_for(s, F, seed):
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    base = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
    return base[None] + np.random.default_rng(seed).normal(scale=0.3, size=(F, n, 3))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # (every call ends in a download: the device has drained)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "max_ms": round(max(ts), 3), "repeats": reps}


def laps_of(fn) -> tuple:
    """The `timing` laps one call prints on stderr: ({lap: ms}, the kernels' ms from events or None)."""
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
    laps, kernel = {}, None
    for line in text.splitlines():
        m = re.match(r"\s*autocorr (\S+)\s+([0-9.]+) ms", line)
        if m and m.group(1).startswith("k_acf"):
            kernel = float(m.group(2))
        elif m:
            laps[m.group(1)] = laps.get(m.group(1), 0.0) + float(m.group(2))
    return laps, kernel


def on_row_blocks(route, m: np.ndarray, *args) -> np.ndarray:
    """route(rows of m, *args) on HOST_THREADS row blocks at once (numpy releases the GIL inside its loops), stacked in row order."""
    edges = np.linspace(0, m.shape[0], min(HOST_THREADS, max(m.shape[0], 1)) + 1).astype(int)
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        parts = list(ex.map(lambda k: route(m[edges[k]:edges[k + 1]], *args), range(len(edges) - 1)))
    return np.concatenate(parts, 0)


def numpy_per_lag(m: np.ndarray, lags, continuous: bool) -> np.ndarray:
    F = m.shape[1]
    out = np.zeros((m.shape[0], len(lags)), np.uint32)
    if continuous:  # (lags must be 0, 1, 2, ...)
        y = m
        for k, t in enumerate(lags):
            if t:
                y = y[:, :-1] & m[:, t:]
            out[:, k] = y.sum(1)
        return out
    for k, t in enumerate(lags):
        out[:, k] = (m[:, :F - t] & m[:, t:]).sum(1)
    return out


def fft_autocorr(m: np.ndarray, L: int) -> np.ndarray:
    R, F = m.shape
    n = 1 << int(np.ceil(np.log2(2 * F)))
    out = np.zeros((R, L + 1), np.uint32)
    block = max(1, (1 << 22) // n)  # (rows per transform: the f64 spectra of a block stay in cache)
    for r0 in range(0, R, block):
        x = np.fft.rfft(m[r0:r0 + block].astype(np.float64), n, axis=1)
        out[r0:r0 + block] = np.rint(np.fft.irfft(x * np.conj(x), n, axis=1)[:, :L + 1]).astype(np.uint32)
    return out


def runs_continuous(m: np.ndarray, L: int) -> np.ndarray:
    """hist[r, n] = runs of length n in row r; acf[t] = sum over n > t of (n - t) hist[n] = S1[t] - t S0[t] with the two suffix sums."""
    R, F = m.shape
    pad = np.zeros((R, F + 2), np.int8)
    pad[:, 1:-1] = m
    d = np.diff(pad, axis=1)
    r_s, s = np.nonzero(d == 1)
    r_e, e = np.nonzero(d == -1)  # (row-major order: the k-th start and the k-th end are one run)
    length = e - s
    hist = np.bincount(r_s * (F + 1) + length, minlength=R * (F + 1)).reshape(R, F + 1).astype(np.int64)
    s0 = hist[:, ::-1].cumsum(1)[:, ::-1]
    s1 = (hist * np.arange(F + 1))[:, ::-1].cumsum(1)[:, ::-1]
    t = np.arange(L + 1)
    return (s1[:, 1:L + 2] - t * s0[:, 1:L + 2]).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=5, type=int)
    ap.add_argument("--label", default="")
    ap.add_argument("--cases", default="1ubq:1000,1ubq:10000,6bft:1000")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    ctx = aa.Context(0)
    lines = []

    def emit(r):
        if a.label:
            r = dict(label=a.label, **r)
        print(json.dumps(r), flush=True)
        lines.append(r)

    for name, F in [(c.split(":")[0], int(c.split(":")[1])) for c in a.cases.split(",")]:
        s = aa.load_model(str(ROOT / "tests" / "data" / f"{name}.pdb"))
        frames = frames_for(s, F, seed=F)
        for level in ("atom", "residue"):
            tl = lambda: ctx.contact_timelines(s, frames, "/", level=level, bitmap=False)
            for _ in range(2):
                tl()
            floor = timed(tl, a.reps)
            masks = None
            for mode in ("intermittent", "continuous"):
                for L in (F - 1, 100):
                    call = lambda: ctx.contact_autocorrelation(s, frames, "/", level=level, mode=mode, max_lag=L)
                    for _ in range(2):
                        got = call()
                    R, W = int(len(got["n_frames"])), (F + 31) // 32
                    r = {"structure": name, "frames": F, "atoms_per_frame": int(frames.shape[1]), "level": level, "mode": mode, "max_lag": L, "rows": R, "words_per_row": W,
                         "matrix_bytes": int(got["autocorrelation"].nbytes), "autocorrelation": timed(call, a.reps), "timelines_no_bitmap": floor}
                    r["over_timelines"] = round(r["autocorrelation"]["best_ms"] / floor["best_ms"], 3)
                    bare = lambda: ctx.contact_autocorrelation(s, frames, "/", level=level, mode=mode, max_lag=L, matrix=False)
                    bare()
                    r["no_matrix"] = timed(bare, a.reps)
                    laps, kernel = laps_of(call)
                    r["laps_ms"] = {k: round(v, 3) for k, v in laps.items()}
                    if kernel:
                        r["kernels_ms"] = round(kernel, 4)
                        if mode == "intermittent":
                            word_lags = R * sum(W - t // 32 for t in range(L + 1))
                            rate = word_lags / (kernel * 1e-3)
                            r["word_lags"] = word_lags
                            r["gword_lags_per_s"] = round(rate / 1e9, 2)
                            r["share_of_vector_ceiling"] = round(rate * INSTR_PER_WORD_LAG / CEILING_LANE_OPS, 4)
                    if not a.no_host:
                        if masks is None:
                            masks = aa.unpack_timeline(ctx.contact_timelines(s, frames, "/", level=level, bitmap=True)["timeline_words"], F)
                        cont = mode == "continuous"
                        t0 = time.perf_counter()
                        probe = on_row_blocks(numpy_per_lag, masks, [0, 1], cont)
                        per_lag = (time.perf_counter() - t0) / 2
                        del probe
                        if per_lag * (L + 1) < 10.0:
                            t0 = time.perf_counter()
                            want = on_row_blocks(numpy_per_lag, masks, list(range(L + 1)), cont)
                            r["numpy_per_lag"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "extrapolated": False,
                                                  "equal_counts": bool(np.array_equal(want, got["autocorrelation"]))}
                        else:
                            some = list(range(32)) if cont else sorted(set(np.linspace(0, L, 32).astype(int).tolist()))
                            t0 = time.perf_counter()
                            want = on_row_blocks(numpy_per_lag, masks, some, cont)
                            dt = time.perf_counter() - t0
                            r["numpy_per_lag"] = {"ms": round(dt / len(some) * (L + 1) * 1e3, 1), "extrapolated": True, "lags_run": len(some),
                                                  "equal_counts": bool(np.array_equal(want, got["autocorrelation"][:, some]))}
                        fast = runs_continuous if cont else fft_autocorr
                        on_row_blocks(fast, masks, L)
                        t0 = time.perf_counter()
                        want = on_row_blocks(fast, masks, L)
                        r["fast_host"] = {"route": "run histogram + suffix sums" if cont else "rfft", "ms": round((time.perf_counter() - t0) * 1e3, 1),
                                          "equal_counts": bool(np.array_equal(want, got["autocorrelation"]))}
                        # the host routes start from the bitmap the timeline call hands out: its cost is the floor both sides share
                        # what the call adds to the floor is a difference of two best-ofs: a ratio is recorded only where it stands clear of the floor's own spread
                        added = r["autocorrelation"]["best_ms"] - floor["best_ms"]
                        spread = floor["max_ms"] - floor["best_ms"]
                        r["added_to_floor_ms"] = round(added, 3)
                        r["floor_spread_ms"] = round(spread, 3)
                        if added > 2.0 * spread:
                            r["fast_host_over_added"] = round(r["fast_host"]["ms"] / added, 1)
                            r["numpy_per_lag_over_added"] = round(r["numpy_per_lag"]["ms"] / added, 1)
                    del got
                    emit(r)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
