"""Case generators and exact references for the edges of the atom-SASA kernel (k_sasa) and of the SAP neighbour sum (k_neighbor_sum).
No product imports: tests/test_sasa_edge_host.py checks these cases on the CPU, tests/test_sasa_edge_gpu.py and tests/test_sap_sum_edge_gpu.py
run them on the device.

SASA.  The contract (include/arpeggia_amd.h "atom SASA") decides "point k of atom i is buried by j" as d^2 < R_j^2 in f64 from the f32 inputs.
exact_margin() evaluates d^2 - R_j^2 over the rationals (fractions.Fraction; every f32 is a dyadic rational), so it shares no rounding with
the kernel or with tests/sasa_restatement.py.  The f64 chain of the contract is within a few 2^-53 of the exact value relative to R_j^2;
a case whose |margin| is above 2^-40 R_j^2 is therefore decided by exact arithmetic, and the generators report every case that is not.

Neighbour sum.  Coordinates are multiples of 2^-8 below 2^12 and weights multiples of 1/8 in [-1, 1]: every operation of the f64 squared
distance and every f32 partial sum of a few thousand terms is exact, in any order, so the device result must equal the reference bit for bit.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
from scipy.spatial import cKDTree

OFFSETS = (0.0, 100.0, 5000.0, 50000.0)
OFFSET_SIGNS = ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (-1.0, 1.0, -1.0), (1.0, -1.0, -1.0))  # one direction per offset: its draws stay a lattice apart
UNDECIDED = Fraction(1, 2 ** 40)  # x R_j^2: below this exact arithmetic does not speak for the f64 chain


def f32(v) -> np.ndarray:
    return np.asarray(v, np.float64).astype(np.float32)


def _q(v) -> Fraction:
    return Fraction(float(np.float32(v)))


def exact_margin(ci, cj, s_k, R_i, R_j) -> Fraction:
    """d^2 - R_j^2 with t = (c_i - c_j) + s_k R_i per axis, over the rationals, from the f32 values of the arguments.
    Point k of atom i is buried by j iff the margin is below zero."""
    ri, rj = _q(R_i), _q(R_j)
    d2 = Fraction(0)
    for a in range(3):
        t = (_q(ci[a]) - _q(cj[a])) + _q(s_k[a]) * ri
        d2 += t * t
    return d2 - rj * rj


def decided(margin: Fraction, R_j) -> bool:
    rj = _q(R_j)
    return abs(margin) > UNDECIDED * rj * rj


def exact_pair_counts(c, R, sphere):
    """Open-point counts [count_0, count_1] of two atoms alone (c: 2 x 3 f32, R: 2 f32) by exact arithmetic, and the number of (atom, point)
    decisions that exact arithmetic cannot make (|margin| <= 2^-40 R_j^2)."""
    counts, undecided = [], 0
    for i, j in ((0, 1), (1, 0)):
        open_points = 0
        for s_k in sphere:
            m = exact_margin(c[i], c[j], s_k, R[i], R[j])
            undecided += not decided(m, R[j])
            open_points += not (m < 0)
        counts.append(open_points)
    return counts, undecided


def step_f32(v, steps: int) -> np.float32:
    """v moved by `steps` f32 steps (negative: towards -inf)."""
    v = np.float32(v)
    for _ in range(abs(steps)):
        v = np.nextafter(v, np.float32(np.inf if steps > 0 else -np.inf), dtype=np.float32)
    return v


# ---- near-sphere placements ----------------------------------------------------------------------------------------------------------------
def near_sphere_placements(sphere, n_draws: int = 300, seed: int = 20261017, spacing: float = 64.0) -> list:
    """n_draws x 7 two-atom placements: atom j sits where point k of atom i lies on j's sphere, c_j = f32(c_i + s_k R_i + u R_j), walked
    -3 .. +3 f32 steps along the dominant axis of u.  Draw d has its own site of a lattice of `spacing` A (site d), shifted by one of OFFSETS
    on every axis (OFFSET_SIGNS), so placements of different draws never interact and may share a call.  Radii are R = radius + probe
    already (use them with probe 0).  Each placement: dict(c [2, 3] f32, R [2] f32, k, offset, step, draw, margin Fraction)."""
    rng = np.random.default_rng(seed)
    s64 = np.asarray(sphere, np.float32).astype(np.float64)
    out = []
    for d in range(n_draws):
        Ri, Rj = (np.float32(v) for v in rng.uniform(1.0, 4.0, 2))
        k = int(rng.integers(len(s64)))
        off = OFFSETS[d % len(OFFSETS)]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        site = np.array([d % 8, (d // 8) % 8, d // 64], np.float64) * spacing
        ci = f32(np.array(OFFSET_SIGNS[d % len(OFFSETS)]) * off + site + rng.uniform(-1.0, 1.0, 3))
        cj0 = f32(ci.astype(np.float64) + s64[k] * float(Ri) + u * float(Rj))
        axis = int(np.argmax(np.abs(u)))
        for step in range(-3, 4):
            cj = cj0.copy()
            cj[axis] = step_f32(cj0[axis], step)
            out.append({"c": np.stack([ci, cj]), "R": np.array([Ri, Rj], np.float32), "k": k, "offset": off, "step": step, "draw": d,
                        "margin": exact_margin(ci, cj, sphere[k], Ri, Rj)})
    return out


def placement_batches(placements: list) -> list:
    """Calls that hold many placements at once: per (offset, step) the placements of that offset (extent: the lattice, a few hundred A -- the
    kernel's f32 band is narrow) and per step the placements of all offsets (extent 5 x 10^4 A: the band is wide).  One placement per draw in
    a call, so that no two pairs of a call are near each other (checked here).  Returns [(name, c [2 P, 3] f32, R [2 P] f32, placements)]."""
    out = []
    for step in range(-3, 4):
        same_step = [p for p in placements if p["step"] == step]
        groups = [(f"offset{int(off)}_step{step:+d}", [p for p in same_step if p["offset"] == off]) for off in OFFSETS]
        groups.append((f"mixed_step{step:+d}", same_step))
        for name, ps in groups:
            c = np.concatenate([p["c"] for p in ps]).astype(np.float32)
            R = np.concatenate([p["R"] for p in ps]).astype(np.float32)
            near = cKDTree(c.astype(np.float64)).query_pairs(2.0 * float(R.max()) + 1.0, output_type="ndarray")
            assert len(near) == len(ps) and (near[:, 0] // 2 == near[:, 1] // 2).all(), "pairs of one call must not interact"
            out.append((name, c, R, ps))
    return out


# ---- point 0 = (0, 0, 1): centres on z ----------------------------------------------------------------------------------------------------
ON_AXIS_RADII = [(2.0, 2.0, 1.0), (1.5, 1.5, 0.0), (1.7, 1.7, 1.4), (0.5, 10.0, 0.0), (10.0, 0.5, 0.0), (1.2, 2.0, 1.4), (2.0, 1.2, 1.4)]
ON_AXIS_Z = (0.0, -37.5, 100.0, 5000.0, 50000.0)


def on_axis_cases() -> list:
    """Atom i at (x0, y0, z0), atom j straight above it at z0 + (R_i + R_j) rounded to f32, and one f32 step either side.  Point 0 of i is
    (0, 0, 1) R_i above c_i for every n_points, so where the sum is representable t = (0, 0, -R_j) exactly: d^2 == R_j^2, not buried (the
    test is strict); one step closer it is buried.  `swap` lists j first (the pair in the other index order).  Each case: dict(x, y, z f64
    arrays, radius f32, probe, step, touch: the centre distance is exactly R_i + R_j, swap, home: index of atom i, margin Fraction)."""
    out = []
    for ri, rj, probe in ON_AXIS_RADII:
        Ri, Rj = (np.float32(np.float32(r) + np.float32(probe)) for r in (ri, rj))
        for z0 in ON_AXIS_Z:
            want = Fraction(z0) + _q(Ri) + _q(Rj)
            zj0 = np.float32(float(want))
            representable = Fraction(float(zj0)) == want
            for step in (-1, 0, 1):
                zj = step_f32(zj0, step)
                for swap in (False, True):
                    ci, cj = f32([1.25, -2.5, z0]), f32([1.25, -2.5, float(zj)])
                    order = [1, 0] if swap else [0, 1]
                    c = np.stack([ci, cj])[order].astype(np.float64)
                    out.append({"x": c[:, 0], "y": c[:, 1], "z": c[:, 2], "radius": np.array([ri, rj], np.float32)[order], "probe": probe,
                                "R": np.array([Ri, Rj], np.float32)[order], "step": step, "touch": representable and step == 0,
                                "representable": representable, "swap": swap, "home": 1 if swap else 0,
                                "margin": exact_margin(ci, cj, (0.0, 0.0, 1.0), Ri, Rj)})
    return out


# ---- neighbour counts (which atoms make k_sasa flush its 256-entry list) -----------------------------------------------------------------
def neighbour_counts(x, y, z, R, chunk: int = 2000) -> np.ndarray:
    """Per atom the number of other atoms with |c_i - c_j| < R_i + R_j (f64 on the f32 coordinates): every one of them can bury a point of
    i, and the kernel's list holds a superset of them."""
    c = np.stack([f32(x), f32(y), f32(z)], 1).astype(np.float64)
    Rd = np.asarray(R, np.float32).astype(np.float64)
    tree = cKDTree(c)
    out = np.zeros(len(c), np.int64)
    for a in range(0, len(c), chunk):
        nb = tree.query_ball_point(c[a:a + chunk], r=Rd[a:a + chunk] + Rd.max())
        for k, v in enumerate(nb):
            i = a + k
            j = np.asarray(v, np.int64)
            d = np.sqrt(((c[j] - c[i]) ** 2).sum(1))
            out[i] = int(((d < Rd[i] + Rd[j]) & (j != i)).sum())
    return out


def homes_sample(counts, n_top: int, n_random: int, seed: int = 7) -> np.ndarray:
    """Home atoms for the restatement on a large input: the n_top atoms with the most neighbours + n_random others (sorted, distinct)."""
    counts = np.asarray(counts)
    top = np.argsort(-counts, kind="stable")[:n_top]
    rest = np.setdiff1d(np.arange(len(counts)), top)
    rnd = np.random.default_rng(seed).choice(rest, min(n_random, len(rest)), replace=False)
    return np.sort(np.concatenate([top, rnd])).astype(np.int64)


def coincident(n: int, R: float = 3.25):
    """n atoms of equal radius at one place: every test of every point sits on d^2 = |s_k|^2 R^2 ~ R^2."""
    return np.full(n, 12.25), np.full(n, -3.5), np.full(n, 7.125), np.full(n, R, np.float32)


# ---- dyadic clouds for the neighbour sum ----------------------------------------------------------------------------------------------------
SCALE = 256  # coordinates are integers / 2^8


def dyadic_cloud(n: int, side: int, seed: int, lattice: bool) -> dict:
    """n atoms in [0, side)^3 (side <= 4096): coordinates multiples of 2^-8 (lattice: integers; sites may repeat -- coincident atoms);
    weights multiples of 1/8 in [-1, 1] with exact zeros; a random side-chain mask.  q: the coordinates x 2^8 as int64."""
    assert side <= 4096
    rng = np.random.default_rng(seed)
    q = (rng.integers(0, side, (n, 3)) * SCALE if lattice else rng.integers(0, side * SCALE, (n, 3))).astype(np.int64)
    w = (rng.integers(-8, 9, n) / 8.0).astype(np.float32)
    w[rng.random(n) < 0.15] = 0.0
    xyz = q.astype(np.float64) / SCALE
    return {"q": q, "x": xyz[:, 0].copy(), "y": xyz[:, 1].copy(), "z": xyz[:, 2].copy(), "w": w, "side": rng.random(n) < 0.7}


def r_squared(r) -> float:
    """The radius as the engine squares it (reference src/sap.rs:183): the product is formed in f32."""
    return float(np.float32(r) * np.float32(r))


def candidate_pairs(cloud: dict, r_largest: float):
    """Pairs (a < b, indices into the side-chain atoms) within a little more than r_largest, and their exact squared distance x 2^16."""
    idx = np.flatnonzero(cloud["side"])
    q = cloud["q"][idx]
    pairs = cKDTree(q.astype(np.float64) / SCALE).query_pairs(np.sqrt(r_squared(r_largest)) * (1 + 1e-6) + 1e-6, output_type="ndarray")
    d = q[pairs[:, 0]] - q[pairs[:, 1]]
    return idx, pairs, (d * d).sum(1)


def neighbor_sum_exact(cloud: dict, r: float, cand):
    """For every side-chain atom the sum of the weights of the side-chain atoms with d^2 <= f64(f32(r) f32(r)), itself included; 0 for the
    others.  int64 distances, f64 sums of multiples of 1/8 (exact), rounded to f32 (exact).  Also returns the number of pairs that sit
    exactly on the edge d^2 == r^2 and the largest neighbour count."""
    idx, pairs, d2 = cand
    thr = r_squared(r) * SCALE * SCALE  # (a power-of-two scaling: exact; d2 < 2^53 converts exactly)
    inside = d2 <= thr
    a, b = pairs[inside, 0], pairs[inside, 1]
    wd = cloud["w"].astype(np.float64)[idx]
    m = len(idx)
    total = wd + np.bincount(a, wd[b], m) + np.bincount(b, wd[a], m)
    most = 1 + int((np.bincount(a, minlength=m) + np.bincount(b, minlength=m)).max(initial=0))
    assert most < 2 ** 20  # every partial sum is a multiple of 1/8 below 2^20: exact in f32
    out = np.zeros(len(cloud["w"]), np.float32)
    out[idx] = total.astype(np.float32)
    assert np.array_equal(out[idx].astype(np.float64), total)
    return out, int((d2 == thr).sum()), most


# (n atoms, lattice, side, radii; the first radius is the largest: its candidate pairs serve the others).  arp_sap_neighbor_sum gives a task
# of 64 atoms nine waves below 3072 tasks = 196 608 atoms and three from there on.
SQRT5, SQRT2 = float(np.float32(np.sqrt(5.0))), float(np.float32(np.sqrt(2.0)))
# f32(sqrt 3) and f32(sqrt 13) lie below the roots, yet their f32 squares round up to 3.0 and 13.0: the lattice pairs at d^2 = 3 and d^2 = 13
# are in because the product is formed in f32 (formed in f64 it stays below and they would be out)
SQRT3, SQRT13 = float(np.float32(np.sqrt(3.0))), float(np.float32(np.sqrt(13.0)))
SUM_CLOUDS = [
    ("lattice_60k", 60_000, True, 40, (5.0, 3.0, SQRT13, SQRT5, SQRT3, SQRT2, 0.0)),
    ("lattice_60k_sparse", 60_000, True, 120, (13.0,)),
    ("dyadic_60k", 60_000, False, 100, (13.0, 5.0, 3.0)),
    ("lattice_230k", 230_000, True, 64, (3.0, SQRT5, SQRT3, SQRT2, 0.0)),
    ("lattice_230k_mid", 230_000, True, 110, (5.0,)),
    ("lattice_230k_sparse", 230_000, True, 300, (13.0,)),
    ("dyadic_230k", 230_000, False, 160, (5.0, 3.0)),
]
SPLIT3_FROM = 3072 * 64


def sum_cloud(name: str) -> dict:
    k = [c[0] for c in SUM_CLOUDS].index(name)
    _, n, lattice, side, _ = SUM_CLOUDS[k]
    return dyadic_cloud(n, side, 4100 + k, lattice)
