"""Helpers of the ensemble SASA / SAP tests (arp_sasa_ensemble): the contract's aggregate formulas restated with Python integers and numpy,
and the per-frame loop over the existing entry points that the device path is held to."""
from __future__ import annotations

import math

import numpy as np

import arpeggia_amd as aa
from arpeggia_amd import _lib

FOUR_PI = 4.0 * 3.141592653589793
BACKBONE = [b"N", b"CA", b"C", b"O", b"OXT"]
SAP_TOL = 2e-5  # x max(1, max |want|): tests/test_sasa_gpu.py test_sap_matches_the_restatement -- the same f32 sum in another order


def vdw(elements) -> np.ndarray:
    p = aa.default_params()
    return np.array([p.vdw_radius[_lib.lib.arp_element_class(e)] for e in elements], dtype=np.float32)


def topology_xyz(s: aa.Structure) -> np.ndarray:
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    return np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)


def jittered(s: aa.Structure, n_frames: int, seed: int, sigma: float = 0.3) -> np.ndarray:
    """As tests/test_freq_gpu.py: every atom of the topology moved by a seeded normal step per frame."""
    base = topology_xyz(s)
    rng = np.random.default_rng(seed)
    return base[None] + rng.normal(scale=sigma, size=(n_frames,) + base.shape)


def sasa_stats(n_frames: int, R, n_points: int, counts) -> dict:
    """include/arpeggia_amd.h arp_sasa_ensemble: S1, S2, D = F S2 - S1^2 as Python integers; every value one f64 chain, left to right,
    rounded to f32 once.  counts: [F, m] integers."""
    counts = np.asarray(counts)
    F, m = counts.shape
    assert F == n_frames
    out = {k: np.zeros(m, np.float32) for k in ("mean_sasa", "std_sasa", "min_sasa", "max_sasa")}
    n, Ff = float(n_points), float(n_frames)
    for k in range(m):
        col = [int(c) for c in counts[:, k]]
        s1, s2 = sum(col), sum(c * c for c in col)
        d = n_frames * s2 - s1 * s1
        assert d >= 0
        r = float(np.float32(R[k]))
        b = (FOUR_PI * r) * r
        out["mean_sasa"][k] = np.float32(b * float(s1) / n / Ff)
        out["std_sasa"][k] = np.float32(b * math.sqrt(float(d)) / n / Ff)
        out["min_sasa"][k] = np.float32(b * float(min(col)) / n)
        out["max_sasa"][k] = np.float32(b * float(max(col)) / n)
    return out


def sap_stats(sap) -> dict:
    """T1, T2: f64 sums of the per-frame f32 values and of their squares, added in frame order; mu = T1 / F; std = sqrt(max(T2 / F - mu mu, 0))."""
    sap = np.asarray(sap, np.float32)
    F, m = sap.shape
    t1, t2 = np.zeros(m, np.float64), np.zeros(m, np.float64)
    for f in range(F):
        d = sap[f].astype(np.float64)
        t1 = t1 + d
        t2 = t2 + d * d
    mu = t1 / float(F)
    var = t2 / float(F) - mu * mu
    return {"mean_sap": mu.astype(np.float32), "std_sap": np.sqrt(np.where(var > 0.0, var, 0.0)).astype(np.float32),
            "min_sap": sap.min(0), "max_sap": sap.max(0), "t1": t1, "t2": t2}


def total_sasa(sasa) -> np.ndarray:
    """Per frame: the f64 sum of the f32 values in atom order (cumsum adds one by one), rounded to f32."""
    sasa = np.asarray(sasa, np.float32)
    return np.array([np.cumsum(row.astype(np.float64))[-1] if len(row) else 0.0 for row in sasa], np.float64).astype(np.float32)


def frame_loop(ctx, s: aa.Structure, sel, frames, probe: float, n_points: int, sap_radius=None, which=None) -> dict:
    """The existing per-frame entry points on the selected atoms, one frame at a time: aa.atom_sasa, then aa.sap_weight and
    aa.sap_neighbor_sum over the side-chain atoms.  which: frame indices (default all).  Returns [len(which), m] arrays."""
    sel = np.asarray(sel, np.int64)
    r = vdw(s.strings("element")[sel])
    resn = [v.decode() for v in s.strings("resn")[sel]]
    side = ~np.isin(s.strings("atomn")[sel], BACKBONE)
    which = range(len(frames)) if which is None else which
    counts, sasas, saps = [], [], []
    for f in which:
        x, y, z = (np.ascontiguousarray(frames[f][sel, k]) for k in range(3))
        sasa, count = aa.atom_sasa(ctx, x, y, z, r, None, probe, n_points)
        counts.append(count)
        sasas.append(sasa)
        if sap_radius is not None:
            w = np.array([aa.sap_weight(resn[k], float(sasa[k])) for k in range(len(sel))], np.float32)
            saps.append(aa.sap_neighbor_sum(ctx, x, y, z, side, w, sap_radius))
    m = len(sel)
    out = {"count": np.array(counts, np.int32).reshape(len(counts), m), "sasa": np.array(sasas, np.float32).reshape(len(sasas), m),
           "R": (r + np.float32(probe)).astype(np.float32), "side": side}
    if sap_radius is not None:
        out["sap"] = np.array(saps, np.float32).reshape(len(saps), m)
    return out


def result_bytes(r: dict) -> bytes:
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in sorted(r) if k != "n_frames")
