"""Cases and an independent restatement for the torsion call (arp_torsions: torsion.inl + the host half and the host twin in torsion.cpp, one torsion in
table_dev.h).  No product imports: tests/test_torsion_host.py checks arp_torsions_host, the selection and the input checks on the CPU,
tests/test_torsion_gpu.py compares the device with arp_torsions_host.

restate(quad_xyz, B) is numpy, written from the definition in include/arpeggia_amd.h, and shares no code with the C twin: c, s, a (degrees), state, bin of
every (frame, torsion) of quad_xyz [F, D, 4, 3]; over_frames(...) restates the statistics over the frames (counts, transitions, sums, hist, hist2).

A device-equals-host comparison of bins is only meaningful where no angle is within the rounding of atan2 of a bin edge: atan2 is the one function of the
definition that is not correctly rounded on both sides.  Every case built by case() keeps each angle at least MIN_MARGIN = 10^-6 degrees from every edge of
the bin counts it is run with (asserted there); a jittered case that misses it is built again with the next seed, at most one seed overall may be skipped that
way (asserted).  c <= -0.5 and s >= 0 need no margin: c and s are correctly rounded on both sides.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

import trajectory_shapes as ts

DATA = Path(__file__).resolve().parent / "data"
MIN_MARGIN = 1e-6
DEG = 180.0 / np.pi
SLAB = 32        # torsion.inl kTorsionSlab: frames of a slab of the sums
LDS_BYTES = 65536  # torsion.inl kTorsionLdsBytes: hist2 tables up to it are counted in LDS, larger ones by wave-matched global adds
NAN_BITS = 0x7FC00000


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def bins_of(a: np.ndarray, B: int) -> np.ndarray:
    w = 360.0 / B
    k = np.maximum(np.floor((a + 180.0) / w).astype(np.int64), 0)     # (a quotient below 0: -180 less a rounding, bin 0)
    return np.where(k >= B, k - B, k)


def restate(quad_xyz: np.ndarray, B: int = 0) -> dict:
    q = np.asarray(quad_xyz, np.float64)
    b1, b2, b3 = q[..., 1, :] - q[..., 0, :], q[..., 2, :] - q[..., 1, :], q[..., 3, :] - q[..., 2, :]
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    x = _dot(n1, n2)
    y = np.sqrt(_dot(b2, b2)) * _dot(b1, n2)
    h = np.sqrt(x * x + y * y)
    ok = (h > 0) & np.isfinite(h)
    with np.errstate(invalid="ignore", divide="ignore"):
        c, s = np.where(ok, x / h, 0.0), np.where(ok, y / h, 0.0)
    a = np.where(ok, np.arctan2(y, x) * DEG, np.nan)
    state = np.where(~ok, 0, np.where(c <= -0.5, 2, np.where(s >= 0, 1, 3))).astype(np.uint8)
    out = {"c": c, "s": s, "a": a, "state": state, "defined": ok}
    if B:
        out["bin"] = np.where(ok, bins_of(np.where(ok, a, 0.0), B), -1)
    return out


def over_frames(r: dict, B: int = 0, pairs=None, G: int = 0) -> dict:
    """The statistics over the frames from a restatement r = restate(quad_xyz, B)."""
    st = r["state"]
    F, D = st.shape
    out = {"n_defined": r["defined"].sum(0).astype(np.uint32), "state_counts": np.stack([(st == k).sum(0) for k in range(4)], 1).astype(np.uint32),
           "n_transitions": ((st[1:] != 0) & (st[:-1] != 0) & (st[1:] != st[:-1])).sum(0).astype(np.uint32), "sums": np.stack([r["c"].sum(0), r["s"].sum(0)], 1)}
    if B:
        hist = np.zeros((D, B), np.uint32)
        for d in range(D):
            hist[d] = np.bincount(r["bin"][r["defined"][:, d], d], minlength=B)
        out["hist"] = hist
        if pairs is not None and G:
            h2 = np.zeros((G, B, B), np.uint32)
            for a, b, g in np.asarray(pairs):
                both = r["defined"][:, a] & r["defined"][:, b]
                np.add.at(h2, (g, r["bin"][both, a], r["bin"][both, b]), 1)
            out["hist2"] = h2
    return out


def edge_margin(a: np.ndarray, B: int) -> float:
    """The least distance in degrees of a defined angle from an edge of the B bins."""
    a = np.asarray(a, np.float64)
    a = a[np.isfinite(a)]
    if a.size == 0:
        return np.inf
    u = (a + 180.0) / (360.0 / B)
    return float(np.abs(u - np.round(u)).min() * (360.0 / B))


def decision_margins(quad_xyz: np.ndarray) -> dict:
    r = restate(quad_xyz)
    ok = r["defined"]
    return {"c": float(np.abs(r["c"][ok] + 0.5).min()), "s": float(np.abs(r["s"][ok]).min())}


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------------------------
SKIPPED_SEEDS = []   # (name, seed) of every jittered case that was built again


def gather(frames: np.ndarray, quads: np.ndarray) -> np.ndarray:
    """[F, D, 4, 3] from frames [F, N, 3] and quads [D, 4]."""
    return np.asarray(frames, np.float64)[:, np.asarray(quads, np.int64)]


def clear(frames, quads, bins) -> bool:
    a = restate(gather(frames, quads))["a"]
    return all(edge_margin(a, B) >= MIN_MARGIN for B in bins)


def case(name: str, frames: np.ndarray, quads: np.ndarray, bins=(36,)) -> dict:
    """A case of the device-equals-twin comparison: frames [F, N, 3], quads [D, 4], and the bin counts it is run with; the margins are asserted."""
    frames = np.ascontiguousarray(frames, np.float64)
    quads = np.ascontiguousarray(quads, "<u4").reshape(-1, 4)
    a = restate(gather(frames, quads))["a"]
    for B in bins:
        assert edge_margin(a, B) >= MIN_MARGIN, (name, B, edge_margin(a, B))
    frames.setflags(write=False)
    return {"name": name, "frames": frames, "quads": quads, "bins": tuple(bins)}


def jittered(name: str, base: np.ndarray, quads: np.ndarray, F: int, seed: int, bins=(36,), sigma: float = ts.SIGMA) -> dict:
    """F frames of base [N, 3] with N(0, sigma) per atom, from the first seed >= `seed` whose angles clear the margins of every B in bins."""
    for s in range(seed, seed + 10):
        frames = ts.jitter(base, F, s, sigma)
        if clear(frames, quads, bins):
            if s != seed:
                SKIPPED_SEEDS.append((name, seed))
            assert len(SKIPPED_SEEDS) <= 1, SKIPPED_SEEDS
            return case(name, frames, quads, bins)
    raise AssertionError(f"{name}: no seed in {seed} .. {seed + 9} clears the margins")


# ---- built torsions -------------------------------------------------------------------------------------------------------------------------------------------------
def built(theta_deg: float) -> np.ndarray:
    """[4, 3]: p0 = (1, 0, 0), p1 = 0, p2 = (0, 0, 1), p3 = (cos t, sin t, 1): the torsion is t."""
    t = np.radians(theta_deg)
    return np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [np.cos(t), np.sin(t), 1.0]])


# integer coordinates of p3 for the angles that have them: exactly planar trans and cis, and +-90
BUILT_INTEGER = {0: (1, 0, 1), 180: (-1, 0, 1), 90: (0, 1, 1), -90: (0, -1, 1)}


def built_integer(theta: int) -> np.ndarray:
    q = built(0.0)
    q[3] = BUILT_INTEGER[theta]
    return q


COLLINEAR = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [3.0, 1.0, 0.0]])   # p0, p1, p2 on a line: n1 = 0 and b1 . n2 = 0 exactly


def four_atoms(quad: np.ndarray) -> list:
    """Topology atoms (trajectory_shapes.records) of one residue whose N, CA, C, O sit on the four points."""
    return [("GLY", name, elem, "A", 1, tuple(quad[k])) for k, (name, elem) in enumerate((("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O")))]


def state_frames(states: list) -> np.ndarray:
    """[F, 4, 3]: one built torsion per frame in the given state: 1 -> 65 (g+), 2 -> 175 (t), 3 -> -65 (g-), all in the middle of a 10-degree bin;
    0 -> undefined (p0 = p1)."""
    angle = {1: 65.0, 2: 175.0, 3: -65.0}
    out = []
    for s in states:
        q = built(angle.get(s, 0.0))
        if s == 0:
            q[0] = q[1]
        out.append(q)
    return np.array(out)


def mirrored(frames: np.ndarray) -> np.ndarray:
    m = np.array(frames, np.float64)
    m[..., 0] = -m[..., 0]
    return m
