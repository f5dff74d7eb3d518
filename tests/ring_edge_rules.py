"""A plain restatement of the ring rules (cation - pi, pi - pi) and inputs that sit on their thresholds.  TEST INFRASTRUCTURE ONLY.

The device decides the ring rows in table_dev.hip (fit_plane_dev, cation_pi_d, pi_stacking_d, compare_residues_d, the cell walk of k_ring_atom)
and again per frame in freq_rings.inl; the oracle does it in arp_oracle.c (plane_fit: a one-sided Jacobi, orc_get_contacts).  This module states
the rules a third time, in Python floats and the oracle's operation order (no FMA), with math.acos and the same fold constants, and takes the
PLANES AS INPUT -- centre and normal per ring residue -- so that it can be evaluated on the closed-form planes, on the oracle's and on the
device's.  fit_plane() is a Python port of fit_plane_dev: the same sums, sweep order, stop tests and eigenvalue selection.  It imports neither
the product nor the oracle; the predicates cover only what the motifs use (PHE rings, LYS NZ), groups "/" and one model.

Motifs.  A motif is a chain-A PHE ring and its partners in chain B: one LYS NZ per partner atom, or a second PHE ring.  Motifs of a structure
sit 32 A apart on a cubic lattice, one decision each; the same sweeps are emitted as frames of a one-motif topology at the origin, where a
coordinate ulp moves an angle by about one ulp as well.

Exact planes.  hexagon(c, k) has the six points c +- r e_u, c +- (r/2 e_u + h e_v), c +- (r/2 e_u - h e_v) (u, v the axes other than k,
r = 1.390625, h = f32(r sqrt 3 / 2)): with c on a dyadic grid coarse enough that the six-term coordinate sums are exact (grid_for), the centroid
is c, the centred coordinates are exact, every off-diagonal covariance sum is exactly zero, no Jacobi variant rotates, and the normal is the
unit vector e_k bit for bit -- for the oracle's fit, the device's and the port alike.  Theta and the distances to such a ring depend only on
IEEE subtract, multiply, add, sqrt, divide and one acos.

Families (sweeps(family) -> [Sweep]):
  "a"  cation - pi on exact planes, the normal along x, y, z (the three selection branches of the fit): theta across 30 at -4 .. +4 coordinate
       ulps along an in-plane axis and two diagonals at d = 3.5 and 4.4; d across 4.5 on the axis and off it at theta = 25
  "b"  pi - pi, both rings exact: parallel (dihedral exactly 0) theta across 30 and 60, centre distance across 6; perpendicular (dihedral exactly
       90) theta across 30 from below and across 60, centre distance across 5 (on the axis, where 5.0 itself is reached) and across 6; concentric perpendicular rings (NaN theta: a
       PiTStacking), a cation on the ring centre (0 / 0: no row), theta exactly 90
  "c"  the nearest quotients: for theta = 30 (cation, parallel, perpendicular) and 60 (parallel, perpendicular), on either side of the ring, a
       seeded search over distance and azimuth for geometries whose q = dot / (|n| |v|) IS one of the doubles at which the host's
       fold_deg(acos q) flips `<= T` or `< T` (hunt_targets: found by find_flip); an exact T, where some q gives one, is among them
  "d"  tilted rings (fitted planes): the partner ring turned about y so that the dihedral crosses 30 and 60; delta is bisected on the restatement
       over the ported fit and moved to the next -4 .. +4 values that change a coordinate
  "e"  fit inputs (fitted planes, not exact): 3 ring atoms, altloc twins, next to +-9999 A, 1e-3 A out-of-plane noise, every axis permutation;
       and a cation on the axis of a fitted ring in every permutation: q is 1 or a neighbour of 1, and one ulp above 1 is NaN and no row
  "f3", "f4"  search edges of k_ring_atom with dist_cutoff 3.0 / 4.0: a cation on the axis at exactly the cutoff (a row) and one coordinate ulp
       beyond (none), the motif slid along +-x, +-y, +-z in 0.5 A steps over 8 A; the first and the last motif are the corners of the box
"""
from __future__ import annotations

import functools
import math
import zlib
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

import synth
from edge_rules import find_flip, step

PI, HALF_PI = 3.14159265358979323846, 1.57079632679489661923  # the constants of fold_deg (residues.rs:50-53,70-73)
RAD2DEG = 180.0 / 3.14159265358979323846264338327950288
NAN = math.nan
CODES = {"PiDisplacedStacking": 11, "PiTStacking": 12, "PiSandwichStacking": 13, "PiParallelInPlaneStacking": 14, "PiTiltedStacking": 15,
         "PiLStacking": 16, "CationPi": 17}
SANDWICH, DISPLACED, INPLANE, TILTED, LSTACK, TSTACK, CATION_PI = 13, 11, 14, 15, 16, 12, 17
RING_NAMES = ("CG", "CD1", "CD2", "CE1", "CE2", "CZ")
R_HEX = 1.390625
H_HEX = float(np.float32(R_HEX * math.sqrt(3.0) / 2.0))
SPACING = 32.0
OFFSETS = tuple(range(-4, 5))
FAR = 9999.0

Plane = namedtuple("Plane", "c n")


# ---------------------------------------------------------------------------------------------- plane geometry (arp_oracle.c:807-824)
def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return NAN if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _acos(q):
    return math.acos(q) if -1.0 <= q <= 1.0 else NAN  # (C acos: NaN outside [-1, 1] and for NaN)


def fold_deg(rad):
    if rad > HALF_PI:
        rad = PI - rad
    return rad * RAD2DEG


def norm3(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def point_dist(pl, q):
    return norm3((q[0] - pl.c[0], q[1] - pl.c[1], q[2] - pl.c[2]))


def point_q(pl, q):
    v = (q[0] - pl.c[0], q[1] - pl.c[1], q[2] - pl.c[2])
    dot = pl.n[0] * v[0] + pl.n[1] * v[1] + pl.n[2] * v[2]
    return _div(dot, norm3(pl.n) * norm3(v))


def point_angle(pl, q):
    return fold_deg(_acos(point_q(pl, q)))


def dihedral_q(a, b):
    dot = a.n[0] * b.n[0] + a.n[1] * b.n[1] + a.n[2] * b.n[2]
    return _div(dot, norm3(a.n) * norm3(b.n))


def plane_dihedral(a, b):
    return fold_deg(_acos(dihedral_q(a, b)))


def angle_of_q(q):
    return fold_deg(_acos(q))


# ---------------------------------------------------------------------------------------------- the rules
def find_cation_pi(pl, q):
    """aromatic.rs:14-29: (is a CationPi, distance from the ring centre)."""
    d, theta = point_dist(pl, q), point_angle(pl, q)
    return (theta <= 30.0) and (d <= 4.5), d


def find_pi_pi(p1, p2, dist):
    """aromatic.rs:33-64 for two rings whose centres are `dist` (<= 6) apart: the stacking code or None."""
    theta, dih = point_angle(p1, p2.c), plane_dihedral(p1, p2)
    if dih <= 30.0:
        if theta <= 30.0:
            return SANDWICH
        if theta <= 60.0:
            return DISPLACED
        if theta <= 90.0:
            return INPLANE
    elif dih <= 60.0:
        return TILTED
    elif dih <= 90.0:
        if theta >= 30.0 and theta < 60.0:
            return LSTACK
        if dist <= 5.0:
            return TSTACK
    return None


ResKey = namedtuple("ResKey", "model chain ord in_l in_r")


def compare_residues(a, b, symmetric):
    """should_compare_residues (complex.rs:94-131)."""
    if a.model != b.model:
        return False
    if not ((a.in_l and b.in_r) or (b.in_l and a.in_r)):
        return False
    if a.chain == b.chain:
        if symmetric:
            return b.ord > 1 and a.ord < b.ord - 1
        neigh = (b.ord in (a.ord, a.ord + 1)) if a.ord == 0 else (b.ord in (a.ord - 1, a.ord, a.ord + 1))
        return not neigh
    return not (symmetric and a.in_r and b.in_r and a.in_l and b.in_l and a.chain > b.chain)


# ---------------------------------------------------------------------------------------------- the fit (table_dev.hip fit_plane_dev)
def fit_plane(pts):
    """Centroid and direction of least variance of [m, 3] points by the device's two-sided cyclic Jacobi; None for fewer than 3 points."""
    pts = [tuple(float(v) for v in p) for p in pts]
    n = len(pts)
    if n < 3:
        return None
    c = [0.0, 0.0, 0.0]
    for p in pts:
        c[0] += p[0]; c[1] += p[1]; c[2] += p[2]
    c = [c[k] / float(n) for k in range(3)]
    A = [[0.0] * 3 for _ in range(3)]
    for p in pts:
        d = (p[0] - c[0], p[1] - c[1], p[2] - c[2])
        for i in range(3):
            for j in range(3):
                A[i][j] += d[i] * d[j]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(64):
        off = abs(A[0][1]) + abs(A[0][2]) + abs(A[1][2])
        diag = abs(A[0][0]) + abs(A[1][1]) + abs(A[2][2])
        if off <= 1e-300 or off <= 1e-18 * diag:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if abs(A[p][q]) <= 1e-300:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                cs = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * cs
                for k in range(3):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = cs * akp - sn * akq; A[k][q] = sn * akp + cs * akq
                for k in range(3):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = cs * apk - sn * aqk; A[q][k] = sn * apk + cs * aqk
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq
    e0, e1, e2 = A[0][0], A[1][1], A[2][2]
    col = 1 if (e1 < e0 and e1 <= e2) else (2 if (e2 < e0 and e2 < e1) else 0)
    v = (V[0][col], V[1][col], V[2][col])
    nn = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return Plane(tuple(c), (v[0] / nn, v[1] / nn, v[2] / nn))


# ---------------------------------------------------------------------------------------------- topology of a records dict
@dataclass
class Topology:
    n: int
    res_key: list       # per residue (file order = hierarchy order: chains are contiguous): (chain, resi)
    res_atoms: list     # per residue: atom indices
    res_ord: list       # per residue: position in its chain
    res_of: list        # per atom
    ring_atoms: list    # per residue: indices of its ring-plane atoms ([] for a residue that is no ring)
    rings: list         # ring entities in order: (residue, altloc)
    cations: list       # atoms that are positively ionizable by residue and atom name (aromatic.rs:18)


def topology(rec) -> Topology:
    n = len(rec["x"])
    index, res_key, res_atoms, res_of = {}, [], [], []
    for k in range(n):
        key = (bytes(rec["chain"][k]), int(rec["resi"][k]))
        if key not in index:
            index[key] = len(res_key)
            res_key.append(key); res_atoms.append([])
        res_atoms[index[key]].append(k)
        res_of.append(index[key])
    seen, res_ord = {}, []
    for ch, _ in res_key:
        res_ord.append(seen.get(ch, 0))
        seen[ch] = res_ord[-1] + 1
    ring_atoms, rings = [], []
    for r, ks in enumerate(res_atoms):
        ra = [k for k in ks if bytes(rec["resn"][k]) == b"PHE" and bytes(rec["name"][k]).decode() in RING_NAMES]
        ring_atoms.append(ra if len(ra) >= 3 else [])
        if len(ra) >= 3:
            rings += [(r, alt) for alt in dict.fromkeys(bytes(rec["altloc"][k]) for k in ks)]
    cations = [k for k in range(n) if bytes(rec["resn"][k]) == b"LYS" and bytes(rec["name"][k]) == b"NZ"]
    return Topology(n, res_key, res_atoms, res_ord, res_of, ring_atoms, rings, cations)


def port_planes(top: Topology, xyz) -> dict:
    """{residue: Plane} of every ring residue by the ported fit."""
    return {r: fit_plane([xyz[k] for k in ra]) for r, ra in enumerate(top.ring_atoms) if ra}


def ring_rows(top: Topology, xyz, planes: dict, cutoff: float) -> set:
    """The ring rows of get_contacts (complex.rs:301-405) for groups "/" and one model, on the given planes:
    {(from entity, to entity, code, f32 distance bits)}, entity = atom index or n + ring entity index."""
    xyz = [tuple(float(v) for v in p) for p in xyz]
    r2 = cutoff * cutoff
    key = lambda r: ResKey(0, top.res_key[r][0], top.res_ord[r], True, True)
    bits = lambda d: int(np.float32(d).view(np.uint32))
    out = set()
    for e, (r, _) in enumerate(top.rings):
        pl = planes[r]
        for y in top.cations:
            q = xyz[y]
            dx, dy, dz = q[0] - pl.c[0], q[1] - pl.c[1], q[2] - pl.c[2]
            if not (dx * dx + dy * dy + dz * dz <= r2):
                continue
            if not compare_residues(key(r), key(top.res_of[y]), False):
                continue
            hit, d = find_cation_pi(pl, q)
            if hit:
                out.add((top.n + e, y, CATION_PI, bits(d)))
    for e1, (ra, _) in enumerate(top.rings):
        p1 = planes[ra]
        for e2, (rb, _) in enumerate(top.rings):
            p2 = planes[rb]
            if abs(p1.c[0] - p2.c[0]) > 7.0 or abs(p1.c[1] - p2.c[1]) > 7.0 or abs(p1.c[2] - p2.c[2]) > 7.0:
                continue  # (only a shortcut: such centres are more than 6 A apart)
            if not compare_residues(key(ra), key(rb), True):
                continue
            dist = norm3((p1.c[0] - p2.c[0], p1.c[1] - p2.c[1], p1.c[2] - p2.c[2]))
            if not (dist <= 6.0):
                continue
            code = find_pi_pi(p1, p2, dist)
            if code is not None:
                out.add((top.n + e1, top.n + e2, code, bits(dist)))
    return out


# ---------------------------------------------------------------------------------------------- motifs
def axes(k):
    return (k + 1) % 3, (k + 2) % 3


def unit(k, s=1.0):
    v = [0.0, 0.0, 0.0]
    v[k] = s
    return tuple(v)


def hexagon(c, k):
    """The exact-plane hexagon around c with normal e_k; opposite points are neighbours in the list."""
    u, v = axes(k)
    out = []
    for a, b in ((R_HEX, 0.0), (R_HEX / 2.0, H_HEX), (R_HEX / 2.0, -H_HEX)):
        for s in (1.0, -1.0):
            p = list(c)
            p[u] += s * a; p[v] += s * b
            out.append(tuple(p))
    return out


def exact_plane(c, k):
    return Plane(tuple(float(x) for x in c), unit(k))


def grid_for(cmax: float) -> float:
    """The coarsest-needed dyadic grid for ring centres up to |cmax|: six coordinates below cmax + 8 sum without rounding."""
    return 2.0 ** (math.ceil(math.log2(6.0 * (cmax + 8.0))) - 53)


def snap(x, g):
    return round(x / g) * g


@dataclass
class Motif:
    a_pts: list                     # chain-A PHE: [(name, altloc, xyz)]
    partners: list                  # chain B: one residue each: [xyz] (LYS NZ) or six xyz (PHE ring)
    a_plane: Plane | None = None    # closed-form planes (None: a fitted plane)
    b_planes: list = field(default_factory=list)


def ring_atoms_of(c, k):
    return [(nm, "", p) for nm, p in zip(RING_NAMES, hexagon(c, k))]


def rc_motif(C, k, q):
    return Motif(ring_atoms_of(C, k), [[tuple(q)]], exact_plane(C, k), [None])


def rr_motif(C, k, c2, k2):
    return Motif(ring_atoms_of(C, k), [hexagon(c2, k2)], exact_plane(C, k), [exact_plane(c2, k2)])


@dataclass
class Sweep:
    label: str
    n_points: int
    point: object            # point(j, C, g) -> Motif: the j-th point of the sweep with the chain-A ring at C, ring centres on the grid g
    both: bool = True        # the points must show two different outcomes
    exact: bool = True       # closed-form planes


def _flip_on_grid(pred, m_lo, m_hi, g):
    pa = pred(m_lo * g)
    assert pa != pred(m_hi * g), "the bracket does not straddle the boundary"
    while m_hi - m_lo > 1:
        m = (m_lo + m_hi) // 2
        if pred(m * g) == pa:
            m_lo = m
        else:
            m_hi = m
    return m_hi


def _swept(pred_of_point, P, k, j, g):
    """P with coordinate k at the flip of pred_of_point along it, moved by OFFSETS[j] steps (ulps for g None, else grid steps)."""
    P = list(P)

    def pred(x):
        Q = list(P); Q[k] = x
        return pred_of_point(Q)

    span = 1e-6 * (1.0 + abs(P[k]))
    if g is None:
        P[k] = step(find_flip(pred, P[k] - span, P[k] + span), OFFSETS[j])
    else:
        m0, dm = round(P[k] / g), round(span / g)
        P[k] = (_flip_on_grid(pred, m0 - dm, m0 + dm, g) + OFFSETS[j]) * g
    return P


def _dir(k, T_deg, w_uv, d, sign=1.0):
    """d (cos T e_k sign + sin T w), w = the in-plane direction (w_u, w_v) normalised."""
    u, v = axes(k)
    t = math.radians(T_deg)
    wn = math.hypot(*w_uv)
    out = [0.0, 0.0, 0.0]
    out[k] = sign * d * math.cos(t)
    out[u] = d * math.sin(t) * w_uv[0] / wn
    out[v] = d * math.sin(t) * w_uv[1] / wn
    return out


def _add(C, v):
    return [C[0] + v[0], C[1] + v[1], C[2] + v[2]]


def cation_sweep(label, k, T, w_uv, d, coord):
    """LYS NZ at C + d (cos T n + sin T w); coord "u": the in-plane coordinate swept (theta), "k": the normal one (distance)."""
    def point(j, C, g):
        pl = exact_plane(C, k)
        P = _swept(lambda Q: find_cation_pi(pl, Q)[0], _add(C, _dir(k, T, w_uv, d)), axes(k)[0] if coord == "u" else k, j, None)
        return rc_motif(C, k, P)
    return Sweep(label, len(OFFSETS), point)


def ring_sweep(label, k, k2, T, w_uv, d, coord, inside):
    """A second exact ring (normal e_k2) with its centre at C + d (cos T n + sin T w) on the grid; inside: the code on one side of the flip."""
    def point(j, C, g):
        p1 = exact_plane(C, k)

        def pred(Q):
            p2 = exact_plane(Q, k2)
            dist = norm3((p1.c[0] - p2.c[0], p1.c[1] - p2.c[1], p1.c[2] - p2.c[2]))
            return dist <= 6.0 and find_pi_pi(p1, p2, dist) == inside

        P0 = [snap(x, g) for x in _add(C, _dir(k, T, w_uv, d))]
        return rr_motif(C, k, _swept(pred, P0, axes(k)[0] if coord == "u" else k, j, g), k2)
    return Sweep(label, len(OFFSETS), point)


def one(label, make):
    return Sweep(label, 1, lambda j, C, g: make(C), both=False)


# ---------------------------------------------------------------------------------------------- the nearest quotients
@functools.lru_cache(maxsize=None)
def hunt_targets(T: float, sign: int) -> tuple:
    """The doubles q (of the given sign) at which fold_deg(acos q) flips `<= T` or `< T`: two or three neighbours, in the order of falling
    angle for sign +1.  Where some q gives exactly T it is the middle one."""
    q0 = sign * math.cos(math.radians(T))
    out = set()
    for pred in (lambda q: angle_of_q(q) <= T, lambda q: angle_of_q(q) < T):
        b = find_flip(pred, q0 - 1e-9, q0 + 1e-9)
        out |= {step(b, -1), b}
    return tuple(sorted(out))


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def hunt(label, kind, k, k2, T, sign, max_tries=20000):
    """One point per target q: a seeded search over d in [3.2, 4.4] (5.2 .. 5.8 for perpendicular rings, where the centre distance must stay
    above 5) and the azimuth; the normal coordinate is bisected to the flip and its neighbourhood scanned for the target."""
    targets = hunt_targets(T, sign)

    def point(j, C, g):
        pl = exact_plane(C, k)
        rng = np.random.default_rng(_seed(label, j, tuple(C)))
        gg = g if kind == "rr" else None
        for _ in range(max_tries):
            d = rng.uniform(5.2, 5.8) if (kind == "rr" and k2 != k) else rng.uniform(3.2, 4.4)
            phi = rng.uniform(0.0, 2.0 * math.pi)
            P = _add(C, _dir(k, T, (math.cos(phi), math.sin(phi)), d, float(sign)))
            if gg is not None:
                P = [snap(x, gg) for x in P]
            inside = lambda Q: angle_of_q(point_q(pl, Q)) <= T
            span = 1e-6 * (1.0 + abs(P[k]))
            if gg is None:
                x0 = find_flip(lambda x: inside(P[:k] + [x] + P[k + 1:]), P[k] - span, P[k] + span)
                cand = [step(x0, o) for o in range(-12, 13)]
            else:
                m0, dm = round(P[k] / gg), round(span / gg)
                mf = _flip_on_grid(lambda x: inside(P[:k] + [x] + P[k + 1:]), m0 - dm, m0 + dm, gg)
                cand = [(mf + o) * gg for o in range(-12, 13)]
            for x in cand:
                Q = P[:k] + [x] + P[k + 1:]
                if point_q(pl, Q) == targets[j]:
                    return rc_motif(C, k, Q) if kind == "rc" else rr_motif(C, k, Q, k2)
        raise AssertionError(f"{label}: no geometry with q = {targets[j]!r} at {C} in {max_tries} tries")

    return Sweep(label, len(targets), point)


# ---------------------------------------------------------------------------------------------- fit inputs
def _rotation(seed):
    q = np.random.default_rng(seed).normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _fitted(C, local, perm=(0, 1, 2), seed=5, alts=("",), names=RING_NAMES, tilt=10.0):
    """A ring of local coordinates [m, 3] (z = out of plane) turned by a fixed rotation, its axes permuted, around C; a LYS NZ 3.5 A from C,
    `tilt` degrees off the turned z axis (10: far from every threshold; 0: on the axis of the fitted plane, where q lands on 1 or next to it
    and one ulp above 1 is no row)."""
    R = _rotation(seed)
    pts = (np.asarray(local) @ R.T)[:, list(perm)] + np.asarray(C)[None]
    t = math.radians(tilt)
    nz = (np.array([3.5 * math.sin(t), 0.0, 3.5 * math.cos(t)]) @ R.T)[list(perm)] + np.asarray(C)
    a = [(nm, alt, tuple(float(v) for v in p)) for alt in alts for nm, p in zip(names, pts)]
    return Motif(a, [[tuple(float(v) for v in nz)]])


def _local_hexagon():
    phi = np.deg2rad(60.0 * np.arange(6))
    return np.stack([1.39 * np.cos(phi), 1.39 * np.sin(phi), np.zeros(6)], 1)


def fit_sweeps():
    hexa = _local_hexagon()
    noisy = hexa.copy()
    noisy[:, 2] = np.random.default_rng(11).normal(scale=1e-3, size=6)
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    far = lambda s: (lambda C: _fitted((s * (FAR - 8.0), s * (FAR - 8.0), s * (FAR - 8.0)), hexa))
    out = [one("fit three atoms", lambda C: _fitted(C, hexa[[0, 1, 3]], names=("CG", "CD1", "CE1"))),
           one("fit altloc twins", lambda C: _fitted(C, hexa, alts=("A", "B"))),
           one("fit far +", far(1.0)), one("fit far -", far(-1.0)),
           one("fit noisy", lambda C: _fitted(C, noisy))]
    out += [one(f"fit perm {p}", lambda C, p=p: _fitted(C, hexa, perm=p, seed=7)) for p in perms]
    out += [one(f"fit on axis perm {p}", lambda C, p=p: _fitted(C, hexa, perm=p, seed=7, tilt=0.0)) for p in perms]
    # three ring atoms on a line along x: the two smallest eigenvalues are both exactly 0, and the fit's selection (`e1 <= e2`) names y.  The
    # reference's own choice on a tied spectrum is arbitrary: this motif pins the device to the port of its fit, nothing else.
    line = lambda C: Motif([(nm, "", (C[0] + dx, C[1], C[2])) for nm, dx in zip(("CG", "CD1", "CE1"), (-1.5, 0.25, 1.25))], [[(C[0], C[1] + 3.5, C[2])]])
    out.append(one("fit collinear along x", line))
    for s in out:
        s.exact = False
    return out


# ---------------------------------------------------------------------------------------------- tilted rings (fitted planes)
def tilted_hexagon(c2, delta):
    """A regular hexagon of radius 1.39 around c2 whose normal is z turned about y by delta (radians).  Its coordinates are rounded: the plane
    is a fitted one."""
    cd, sd = math.cos(delta), math.sin(delta)
    out = []
    for i in range(6):
        phi = math.radians(60.0 * i)
        a, b = 1.39 * math.cos(phi), 1.39 * math.sin(phi)
        out.append((c2[0] + a * cd, c2[1] + b, c2[2] - a * sd))
    return out


def tilt_sweep(label, T, inside):
    """The partner ring 4 A above ring A (normal z), turned about y so that the dihedral crosses T.  delta is bisected on the restatement over
    the ported fit, then moved to the next -4 .. +4 values of delta that change a coordinate."""
    def point(j, C, g):
        pA = exact_plane(C, 2)
        c2 = (C[0], C[1], C[2] + 4.0)

        def pred(delta):
            pB = fit_plane(tilted_hexagon(c2, delta))
            return find_pi_pi(pA, pB, norm3((pA.c[0] - pB.c[0], pA.c[1] - pB.c[1], pA.c[2] - pB.c[2]))) == inside

        d0 = math.radians(T)
        delta = find_flip(pred, d0 - 1e-6, d0 + 1e-6)
        pts, direction = tilted_hexagon(c2, delta), (1 if OFFSETS[j] > 0 else -1)
        for _ in range(abs(OFFSETS[j])):
            nxt = pts
            while nxt == pts:
                delta = step(delta, direction)
                nxt = tilted_hexagon(c2, delta)
            pts = nxt
        return Motif(ring_atoms_of(C, 2), [pts], exact_plane(C, 2), [None])
    return Sweep(label, len(OFFSETS), point, exact=False)


# ---------------------------------------------------------------------------------------------- search edges
SLIDES = tuple(0.5 * k for k in range(17))
CORNER = 64.0


def _axis_pair(c, k, s, cutoff):
    """(the point at exactly `cutoff` from c along s e_k, the nearest point on the other side that is farther than `cutoff`)."""
    at, beyond = list(c), list(c)
    at[k] = c[k] + s * cutoff
    b = c[k] - s * step(cutoff, 1)
    if abs(b - c[k]) <= cutoff:
        b = step(b, -1 if s > 0 else 1)
    assert abs(at[k] - c[k]) == cutoff and abs(b - c[k]) > cutoff
    beyond[k] = b
    return tuple(at), tuple(beyond)


def search_sweeps(cutoff: float):
    """Per direction +-x, +-y, +-z: the ring at C + slide e_k, a LYS NZ on its axis at exactly `cutoff` (d^2 == cutoff^2: a row) and one on
    the other side one coordinate ulp beyond (no row).  Every coordinate is exact: C, the slides and the cutoffs are dyadic.  The two corner
    motifs lie outside the lattice: their atoms are the smallest (largest) x, y and z of the structure."""
    def slide(k, s):
        def point(j, C, g):
            c = list(C)
            c[k] += s * SLIDES[j]
            at, beyond = _axis_pair(c, k, s, cutoff)
            return Motif(ring_atoms_of(c, k), [[at], [beyond]], exact_plane(c, k), [None, None])
        return Sweep(f"search {cutoff:g} slide {'+' if s > 0 else '-'}{'xyz'[k]}", len(SLIDES), point, both=False)

    def corner(s):
        def point(j, C, g):
            c = [-CORNER if s < 0 else 6.0 * CORNER] * 3
            at, beyond = _axis_pair(c, 0, s, cutoff)  # the cation is the extreme atom along x, the ring's own atoms along y and z
            return Motif(ring_atoms_of(c, 0), [[at], [beyond]], exact_plane(c, 0), [None, None])
        return Sweep(f"search {cutoff:g} corner {'max' if s > 0 else 'min'}", 1, point, both=False)

    return [corner(-1.0)] + [slide(k, s) for k in range(3) for s in (1.0, -1.0)] + [corner(1.0)]


# ---------------------------------------------------------------------------------------------- families
W_DIRS = {"axis": (1.0, 0.0), "diag": (1.0, 1.0), "skew": (2.0, 1.0)}


@functools.lru_cache(maxsize=None)
def sweeps(family: str) -> list:
    out = []
    if family == "a":
        for k in range(3):
            for wn, w in W_DIRS.items():
                for d in (3.5, 4.4):
                    out.append(cation_sweep(f"cation theta 30 n={'xyz'[k]} {wn} d={d}", k, 30.0, w, d, "u"))
            out.append(cation_sweep(f"cation d 4.5 n={'xyz'[k]} on axis", k, 0.0, (1.0, 0.0), 4.5, "k"))
            out.append(cation_sweep(f"cation d 4.5 n={'xyz'[k]} theta 25", k, 25.0, (1.0, 0.0), 4.5, "k"))
    elif family == "b":
        for k in range(3):
            kp = axes(k)[1]  # the perpendicular partner's normal: an in-plane axis of ring A that the sweeps do not move along
            w = list(W_DIRS.values())[k]
            n = "xyz"[k]
            out += [ring_sweep(f"parallel theta 30 n={n}", k, k, 30.0, w, 4.0, "u", SANDWICH),
                    ring_sweep(f"parallel theta 60 n={n}", k, k, 60.0, w, 4.0, "u", DISPLACED),
                    ring_sweep(f"parallel dist 6 n={n}", k, k, 0.0, w, 6.0, "k", SANDWICH),
                    ring_sweep(f"perpendicular theta 30 n={n}", k, kp, 30.0, w, 5.5, "u", LSTACK),
                    ring_sweep(f"perpendicular theta 60 n={n}", k, kp, 60.0, w, 5.5, "u", LSTACK),
                    ring_sweep(f"perpendicular dist 5 n={n}", k, kp, 0.0, w, 5.0, "k", TSTACK),  # on the axis: the distance is 5.0 exactly, then 5.0 + a grid step
                    ring_sweep(f"perpendicular dist 6 n={n}", k, kp, 45.0, w, 6.0, "k", LSTACK)]
        out += [one("concentric perpendicular", lambda C: rr_motif(C, 2, list(C), 0)),
                one("cation on the centre", lambda C: rc_motif(C, 2, list(C))),
                one("theta exactly 90", lambda C: rr_motif(C, 2, [C[0] + 5.0, C[1], C[2]], 2))]
    elif family == "c":
        for sign in (1, -1):
            s = "+" if sign > 0 else "-"
            for k in range(3):
                out.append(hunt(f"hunt cation 30 n={'xyz'[k]} {s}", "rc", k, k, 30.0, sign))
            out += [hunt(f"hunt parallel 30 {s}", "rr", 2, 2, 30.0, sign), hunt(f"hunt parallel 60 {s}", "rr", 0, 0, 60.0, sign),
                    hunt(f"hunt perpendicular 30 {s}", "rr", 1, 2, 30.0, sign), hunt(f"hunt perpendicular 60 {s}", "rr", 2, 0, 60.0, sign)]
    elif family == "d":
        out = [tilt_sweep("tilt dihedral 30", 30.0, SANDWICH), tilt_sweep("tilt dihedral 60", 60.0, TILTED)]
    elif family == "e":
        out = fit_sweeps()
    elif family in ("f3", "f4"):
        out = search_sweeps(3.0 if family == "f3" else 4.0)
    else:
        raise KeyError(family)
    return out


FAMILIES = ("a", "b", "c", "d", "e", "f3", "f4")
TABLE_CUTOFF = {"a": 6.5, "b": 6.5, "c": 6.5, "d": 6.5, "e": 6.5, "f3": 3.0, "f4": 4.0}


# ---------------------------------------------------------------------------------------------- structures and frames
@dataclass
class Built:
    rec: dict
    top: Topology
    motifs: list        # (sweep index, point index, Motif)
    a_res: list         # per motif: its chain-A residue
    b_res: list         # per motif: its chain-B residues
    planes: dict        # {residue: closed-form Plane} for the rings that have one

    @property
    def xyz(self):
        return np.stack([self.rec["x"], self.rec["y"], self.rec["z"]], 1)

    def ring_residues(self, exact: bool):
        return [r for r, ra in enumerate(self.top.ring_atoms) if ra and ((r in self.planes) == exact)]


def _records(motifs) -> Built:
    cols = {k: [] for k in ("x", "y", "z", "occupancy", "serial", "resi", "name", "resn", "chain", "altloc", "icode", "element", "model_serial")}

    def add(resn, name, elem, chain, resi, altloc, xyz):
        k = len(cols["x"])
        for c, v in (("x", xyz[0]), ("y", xyz[1]), ("z", xyz[2]), ("occupancy", 1.0), ("serial", k + 1), ("resi", resi), ("name", name), ("resn", resn),
                     ("chain", chain), ("altloc", altloc), ("icode", ""), ("element", elem), ("model_serial", 0)):
            cols[c].append(v)

    for p, (_, _, m) in enumerate(motifs):
        for nm, alt, q in m.a_pts:
            add("PHE", nm, "C", "A", p + 1, alt, q)
    resi, b_res, n_a = 0, [], len(motifs)
    nb = n_a
    for _, _, m in motifs:
        mine = []
        for part in m.partners:
            resi += 2  # (residues of chain B are no sequence neighbours of each other)
            mine.append(nb)
            nb += 1
            if len(part) == 1:
                add("LYS", "NZ", "N", "B", resi, "", part[0])
            else:
                for nm, q in zip(RING_NAMES, part):
                    add("PHE", nm, "C", "B", resi, "", q)
        b_res.append(mine)
    rec = synth._finish(cols)
    top = topology(rec)
    planes = {}
    for p, (_, _, m) in enumerate(motifs):
        if m.a_plane is not None:
            planes[p] = m.a_plane
        for r, pl in zip(b_res[p], m.b_planes):
            if pl is not None:
                planes[r] = pl
    return Built(rec, top, list(motifs), list(range(n_a)), b_res, planes)


@functools.lru_cache(maxsize=None)
def structure(family: str) -> Built:
    """One structure per family: a motif per sweep point on a cubic lattice from the origin."""
    sw = sweeps(family)
    n = sum(s.n_points for s in sw)
    side = max(1, math.ceil(n ** (1.0 / 3.0) - 1e-9))
    g = grid_for(SPACING * (side - 1))
    motifs, slot = [], 0
    for si, s in enumerate(sw):
        for j in range(s.n_points):
            C = [SPACING * (slot // (side * side)), SPACING * ((slot // side) % side), SPACING * (slot % side)]
            slot += 1
            motifs.append((si, j, s.point(j, C, g)))
    return _records(motifs)


@functools.lru_cache(maxsize=None)
def frames(family: str, si: int):
    """(Built of the sweep's first point at the origin, [F, N, 3] f64): one frame per sweep point, every point made at the origin."""
    s = sweeps(family)[si]
    g = grid_for(0.0)
    motifs = [s.point(j, [0.0, 0.0, 0.0], g) for j in range(s.n_points)]
    built = [_records([(si, j, m)]) for j, m in enumerate(motifs)]
    fr = np.stack([b.xyz for b in built])
    assert all(b.top.rings == built[0].top.rings and b.top.n == built[0].top.n for b in built)
    return built, fr


def outcomes(b: Built, rows: set) -> list:
    """Per motif: the sorted (partner residue, code) of the ring rows that start at its chain-A ring."""
    ent_res = [r for r, _ in b.top.rings]
    per = [[] for _ in b.motifs]
    for frm, to, code, _ in rows:
        r = ent_res[frm - b.top.n]
        if r < len(b.motifs):
            to_res = b.top.res_of[to] if to < b.top.n else ent_res[to - b.top.n]
            per[r].append((to_res - b.b_res[r][0], code))
    return [tuple(sorted(set(x))) for x in per]
