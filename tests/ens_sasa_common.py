"""Helpers of the ensemble SASA / SAP tests (arp_sasa_ensemble): the contract's aggregate formulas restated with Python integers and numpy,
and the per-frame loop over the existing entry points that the device path is held to."""
from __future__ import annotations

import math

import numpy as np

import arpeggia_amd as aa
import bsa_common
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


# ---- what tests/test_ens_sasa_gpu.py and tests/test_ens_shapes_gpu.py assert of a sasa_ensemble result -------------------------------------------
SASA_KEYS = ("mean_sasa", "std_sasa", "min_sasa", "max_sasa")
SAP_KEYS = ("mean_sap", "std_sap", "min_sap", "max_sap")


def assert_sasa_equal(got: dict, want: dict, R, n_points: int):
    """got: the new path with per_frame=True; want: frame_loop over all frames."""
    F = got["n_frames"]
    assert got["count"].dtype == np.int32 and got["count"].shape == want["count"].shape
    assert np.array_equal(got["count"], want["count"])
    stats = sasa_stats(F, R, n_points, want["count"])
    for k in SASA_KEYS:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], stats[k]), k
    # min / max are also the extremes of the loop's own f32 values
    assert np.array_equal(got["min_sasa"], want["sasa"].min(0)) and np.array_equal(got["max_sasa"], want["sasa"].max(0))
    assert np.array_equal(got["total_sasa"], total_sasa(want["sasa"]))


def assert_sap_close(got_sap, want_sap, side):
    assert got_sap.shape == want_sap.shape and got_sap.dtype == np.float32
    assert (got_sap[:, ~side] == 0).all()  # backbone atoms
    tol = SAP_TOL * max(1.0, float(np.abs(want_sap).max(initial=0.0)))
    assert float(np.abs(got_sap - want_sap).max(initial=0.0)) <= tol


def assert_sap_aggregates(got: dict):
    """The aggregation separated from the order tolerance: from the new path's own per-frame values, exactly."""
    w = sap_stats(got["sap"])
    for k in SAP_KEYS:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k


# ---- the per-frame loop of the dSASA form (tests/test_bsa_gpu.py, tests/test_ens_shapes_gpu.py) -------------------------------------------------------
def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def three_runs(ctx, x, y, z, r, group, probe, n_points=100):
    """The existing kernel three times -- the union, group 1 alone, group 2 alone -- laid out as the split kernel's planes."""
    group = np.asarray(group, np.uint8)
    count, sasa = np.zeros((3, len(group)), np.int32), np.zeros((3, len(group)), np.float32)
    for plane, members in enumerate((group != 0, (group & 1) != 0, (group & 2) != 0)):
        s, c = aa.atom_sasa(ctx, x, y, z, r, include=members.astype(np.uint8), probe=probe, n_points=n_points)
        count[plane], sasa[plane] = c, s
    return count, sasa


def bsa_frame_loop(ctx, s, r, frames, probe, n_points):
    """The per-frame loop the ensemble call replaces: three atom_sasa calls per frame and an f64 cumsum per total."""
    sel, group = r["atoms"].astype(np.int64), r["group"]
    radius = (r["R"] - np.float32(probe)).astype(np.float32)
    assert np.array_equal((radius + np.float32(probe)).astype(np.float32), r["R"])
    out = {k: [] for k in ("buried", "total_complex", "total_g1", "total_g2", "dsasa")}
    for f in range(len(frames)):
        x, y, z = (np.ascontiguousarray(frames[f][sel, k]) for k in range(3))
        count, sasa = three_runs(ctx, x, y, z, radius, group, probe, n_points)
        totals = [bsa_common.f64_total(sasa[0]), bsa_common.f64_total(sasa[1][(group & 1) != 0]), bsa_common.f64_total(sasa[2][(group & 2) != 0])]
        out["buried"].append(count[1] + count[2] - count[0])
        for k, v in zip(("total_complex", "total_g1", "total_g2"), totals):
            out[k].append(v)
        out["dsasa"].append(bsa_common.dsasa_f32(*totals))
    return {k: np.array(v) for k, v in out.items()}
