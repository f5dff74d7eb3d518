"""Cases that sit ON the decision thresholds and the launch boundaries of the secondary-structure call (arp_dssp: dssp.inl), with a scalar restatement of the
definition in Python floats.  No product imports: tests/test_dssp_edge_host.py runs them through the host twin and the reach checks on the CPU,
tests/test_dssp_edge_gpu.py through the device call.  (tests/dssp_cases.py keeps its cases 10^-6 away from every threshold; these do not.)

The restatement, restate(x [R, 4, 3], flags), follows the operation order of include/arpeggia_amd.h, every operation one IEEE f64 operation of Python:
  dist = sqrt((dx dx + dy dy) + dz dz);  H = N + (C' - O') / |C' - O'|;  E = 27.888 (((1 / d_ON + 1 / d_CH) - 1 / d_OH) - 1 / d_CN), -9.9 if any of the four
  distances is < 0.5;  cos kappa = dot / (lu lv)
so the expected values are well defined without margins: an input may lie on a threshold, or one ulp to either side of it.

Residues are free point sets: the definition checks nothing inside a residue, which is what makes exact edges possible.  An inert residue has its CA at
(0, 0, 1000 (r + 2)): at least 1000 A from every other CA, so it gets no energy as donor or acceptor, whatever its other atoms do.  Padding residues are inert
and each a chain of its own (chains P and Q in turn).  The active residues of every probe lie within 30 A of the origin.

Launch constants (dssp.inl): TILE = 64 donors per workgroup of the sweep = acceptors per LDS tile = bits of a lane's mask; ASSIGN = 256 lanes stride over the
residues in the assignment; FAR2 = 82 A^2, the prefilter's bound on the squared CA distance.
"""
from __future__ import annotations

import itertools
import math
from functools import lru_cache

import numpy as np

import dssp_cases as dc
import trajectory_shapes as ts

TILE, ASSIGN, FAR2 = 64, 256, 82.0
NONE = 0xFFFFFFFF
HBOND, CA_CUT, BREAK, MIN_DIST, MIN_ENERGY, COUPLING = -0.5, 9.0, 2.5, 0.5, -9.9, 27.888
INF = float("inf")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------------------
def dist(a, b) -> float:
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def hydrogen(n, c_prev, o_prev) -> list:
    ln = dist(c_prev, o_prev)
    return [n[k] + (c_prev[k] - o_prev[k]) / ln for k in range(3)]


def energy(o, c, n, h) -> tuple:
    """(E, the four distances ON, CH, OH, CN) of acceptor (O, C) and donor (N, H)."""
    d_on, d_ch, d_oh, d_cn = dist(o, n), dist(c, h), dist(o, h), dist(c, n)
    if d_on < MIN_DIST or d_ch < MIN_DIST or d_oh < MIN_DIST or d_cn < MIN_DIST:
        return MIN_ENERGY, (d_on, d_ch, d_oh, d_cn)
    return COUPLING * (((1.0 / d_on + 1.0 / d_ch) - 1.0 / d_oh) - 1.0 / d_cn), (d_on, d_ch, d_oh, d_cn)


def cos_kappa(a, b, c) -> float:
    ux, uy, uz, vx, vy, vz = b[0] - a[0], b[1] - a[1], b[2] - a[2], c[0] - b[0], c[1] - b[1], c[2] - b[2]
    dot = (ux * vx + uy * vy) + uz * vz
    lu, lv = math.sqrt((ux * ux + uy * uy) + uz * uz), math.sqrt((vx * vx + vy * vy) + vz * vz)
    return dot / (lu * lv)


def restate(x, flags) -> dict:
    """One frame x [R, 4, 3] (N, CA, C, O): brk, donor, pairs {(i, j): E} of every pair that gets an energy, best [R][2] (acceptor, E) in the definition's order
    (lower E first, the lower index on ties; (NONE, inf) where there is none), hb {(i, j)} and codes [R]."""
    xa = np.asarray(x, np.float64)
    R = len(xa)
    X = xa.tolist()
    N, CA, C_, O = ([X[r][a] for r in range(R)] for a in range(4))
    brk, donor, H = [True] * R, [False] * R, [None] * R
    for r in range(1, R):
        brk[r] = bool(flags[r] & dc.CHAIN_START) or dist(C_[r - 1], N[r]) > BREAK
        donor[r] = not brk[r] and not (flags[r] & dc.NO_H)
        if donor[r]:
            H[r] = hydrogen(N[r], C_[r - 1], O[r - 1])
    # candidates by numpy with a bound far outside any rounding (10 A against the cut of 9); the decision itself is the scalar one below
    ca = xa[:, 1]
    pairs, best = {}, [[(NONE, INF), (NONE, INF)] for _ in range(R)]
    for j in range(R):
        if not donor[j]:
            continue
        d = ca - ca[j]
        found = []
        for i in np.flatnonzero((d * d).sum(1) < 100.0).tolist():
            if i == j or i + 1 == j or not (dist(CA[i], CA[j]) < CA_CUT):
                continue
            e = energy(O[i], C_[i], N[j], H[j])[0]
            pairs[(i, j)] = e
            found.append((e, i))
        found.sort()
        for k, (e, i) in enumerate(found[:2]):
            best[j][k] = (i, e)
    hb = {(i, j) for j in range(R) for i, e in best[j] if i != NONE and e < HBOND}
    return {"brk": brk, "donor": donor, "pairs": pairs, "best": best, "hb": hb, "codes": codes_of(R, brk, hb, CA)}


def codes_of(R: int, brk, hb: set, CA) -> list:
    """The states 0 .. 7 ("-HBEGITS") from the breaks, the bonds (acceptor, donor) and the CA positions, in the definition's order of precedence."""
    def cont(a, b):
        return a >= 0 and b < R and a <= b and not any(brk[r] for r in range(a + 1, b + 1))

    def turn(n, i):
        return cont(i, i + n) and (i, i + n) in hb

    def pairable(i, j):
        return 0 <= i < R and 0 <= j < R and abs(i - j) >= 3 and cont(i - 1, i + 1) and cont(j - 1, j + 1)

    def par(i, j):
        return pairable(i, j) and (((i - 1, j) in hb and (j, i + 1) in hb) or ((j - 1, i) in hb and (i, j + 1) in hb))

    def anti(i, j):
        return pairable(i, j) and (((i, j) in hb and (j, i) in hb) or ((i - 1, j + 1) in hb and (j - 1, i + 1) in hb))

    # every bridge of i with j has a bond between {i - 1, i, i + 1} and {j - 1, j, j + 1}: the partners worth trying
    touch = {}
    for a, b in hb:
        touch.setdefault(a, set()).add(b)
        touch.setdefault(b, set()).add(a)
    code = [0] * R
    for i in range(R):
        cand = {q + s for p in (i - 1, i, i + 1) for q in touch.get(p, ()) for s in (-1, 0, 1)}
        bridge = ladder = False
        for j in sorted(cand):
            p, a = par(i, j), anti(i, j)
            bridge = bridge or p or a
            ladder = ladder or (p and (par(i - 1, j - 1) or par(i + 1, j + 1))) or (a and (anti(i - 1, j + 1) or anti(i + 1, j - 1)))
        code[i] = 3 if ladder else 2 if bridge else 0
    for i in range(R):
        if turn(4, i - 1) and turn(4, i):
            code[i:i + 4] = [1] * 4
    for n, state in ((3, 4), (5, 5)):
        for i in range(R):
            if turn(n, i - 1) and turn(n, i) and all(code[k] in (0, state) for k in range(i, i + n)):
                code[i:i + n] = [state] * n
    for k in range(R):
        if code[k] == 0 and any(turn(n, i) for n in (3, 4, 5) for i in range(k - n + 1, k)):
            code[k] = 6
    for k in range(R):
        if code[k] == 0 and cont(k - 2, k + 2) and cos_kappa(CA[k - 2], CA[k], CA[k + 2]) < dc.COS70:
            code[k] = 7
    return code


def expected(case: dict) -> dict:
    """The call's outputs by the restatement: codes [F, R], counts [R, 8], frame_counts [F, 8], hb_acceptor [F, R, 2], hb_energy f8 [F, R, 2] (unrounded; 0 where
    there is no acceptor), and the per-frame restatements under "frames"."""
    F, R = case["xyz"].shape[:2]
    frames = [restate(case["xyz"][f], case["flags"]) for f in range(F)]
    codes = np.array([fr["codes"] for fr in frames], "u1").reshape(F, R)
    acc = np.array([[[i for i, _ in b] for b in fr["best"]] for fr in frames], "<u4").reshape(F, R, 2)
    en = np.array([[[0.0 if i == NONE else e for i, e in b] for b in fr["best"]] for fr in frames], np.float64).reshape(F, R, 2)
    return {"codes": codes, "counts": np.stack([(codes == k).sum(0) for k in range(8)], 1).astype("<u4"),
            "frame_counts": np.stack([(codes == k).sum(1) for k in range(8)], 1).astype("<u4"), "hb_acceptor": acc, "hb_energy": en, "frames": frames}


def strings(codes) -> list:
    return ["".join(dc.SS[int(c)] for c in row) for row in np.asarray(codes)]


# ---- building blocks --------------------------------------------------------------------------------------------------------------------------------------------------
def ulps(v: float, k: int) -> float:
    """The k-th f64 neighbour of v (k < 0: below)."""
    for _ in range(abs(k)):
        v = math.nextafter(v, INF if k > 0 else -INF)
    return v


def inert_ca(r: int) -> tuple:
    return (0.0, 0.0, 1000.0 * (r + 2))


def pad(r: int) -> list:
    """An inert residue around its far CA."""
    x, y, z = inert_ca(r)
    return [(x - 1.2, y + 0.8, z), (x, y, z), (x + 1.2, y + 0.8, z), (x + 1.2, y + 2.0, z)]


def pad_chain(r: int) -> str:
    return "PQ"[r % 2]


def up(p, dz: float = 1.3) -> tuple:
    """A point within the break distance of p: where the next residue's N goes, or the previous residue's C."""
    return (p[0], p[1], p[2] + dz)


def assemble(R: int, frames: list, chains: dict, resn: dict | None = None) -> dict:
    """frames: per frame {r: [N, CA, C, O]} of the active residues (the same keys in every frame); chains: {r: chain} of the residues that are not padding;
    everything else is padding."""
    assert all(set(fr) <= set(chains) for fr in frames)
    res = [((resn or {}).get(r, "ALA"), chains.get(r, pad_chain(r)), r + 1) for r in range(R)]
    xyz = np.zeros((len(frames), R, 4, 3))
    for f, fr in enumerate(frames):
        for r in range(R):
            xyz[f, r] = fr[r] if r in fr else pad(r)
    case = dc.case_of(res, xyz)
    case["xyz"].setflags(write=False)
    return case


# ---- 1: the turn probe ----------------------------------------------------------------------------------------------------------------------------------------------
def turn_atoms(x=3.0, d=5.0, c2=(-1.0, 1.0, 0.0), o2=(-2.0, 1.0, 0.0), o=None, c=None) -> list:
    """The four residues a .. a + 3 of a turn probe (their rows, a first).  N[a+3] = 0 and H[a+3] = (1, 0, 0) exactly (C[a+2] - O[a+2] = (1, 0, 0)); acceptor a
    has O = (x, 0, 0) and C = (x + 1.23, 0, 0) unless o / c are given; CA[a+3] = (0, -1.5, 0), CA[a] = (d, -1.5, 0): |CA - CA| = d exactly.  a + 1 and a + 2 are
    inert by their CA alone (the caller puts it); their N and C keep the links."""
    o = (x, 0.0, 0.0) if o is None else o
    c = (x + 1.23, 0.0, 0.0) if c is None else c
    r0 = [(d, -3.0, 0.0), (d, -1.5, 0.0), c, o]
    n2 = (-1.0, 2.5, 0.0)
    c1 = up(n2)
    r1 = [up(c), None, c1, up(c1, 1.2)]
    r2 = [n2, None, c2, o2]
    r3 = [(0.0, 0.0, 0.0), (0.0, -1.5, 0.0), (0.0, -3.0, 0.0), (0.0, -4.2, 0.0)]
    return [r0, r1, r2, r3]


def turn_case(variants: list, a: int = 0, trailing: int = 2) -> dict:
    """One frame per entry of variants (keyword arguments of turn_atoms), the probe at residues a .. a + 3 among a pads before and `trailing` after."""
    R = a + 4 + trailing
    frames = []
    for kw in variants:
        rows = turn_atoms(**kw)
        rows[1][1], rows[2][1] = inert_ca(a + 1), inert_ca(a + 2)
        frames.append({a + k: rows[k] for k in range(4)})
    case = assemble(R, frames, {a + k: "A" for k in range(4)})
    case["probe"] = a
    return case


def probe_energy(x: float) -> float:
    rows = turn_atoms(x=x)
    return energy(rows[0][3], rows[0][2], rows[3][0], hydrogen(rows[3][0], rows[2][2], rows[2][3]))[0]


def bisect_flip(pred, lo: float, hi: float) -> tuple:
    """Adjacent doubles (lo, hi) with pred(lo) and not pred(hi), from an interval whose ends differ."""
    assert pred(lo) and not pred(hi)
    while math.nextafter(lo, INF) < hi:
        mid = lo + (hi - lo) / 2.0
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


@lru_cache(maxsize=None)
def energy_edge() -> tuple:
    """(x values of the sweep, x0): x0 and its successor are adjacent doubles between which the restated E < -0.5 flips (E rises through -0.5 near x = 5.124);
    the sweep is x0 and its six neighbours on either side, and every x within 64 neighbours at which E is -0.5 exactly (no bond)."""
    x0, _ = bisect_flip(lambda x: probe_energy(x) < HBOND, 2.9, 7.0)
    xs = [ulps(x0, k) for k in range(-6, 7)]
    xs += [x for x in (ulps(x0, k) for k in range(-64, 65)) if probe_energy(x) == HBOND and x not in xs]
    return tuple(xs), x0


def energy_sweep(a: int = 0, trailing: int = 2) -> dict:
    return turn_case([{"x": x} for x in energy_edge()[0]], a, trailing)


CA_SWEEP = (ulps(9.0, -1), 9.0, ulps(9.0, 1), 9.05, 9.055, 9.06)      # only the first gives a pair; 9 <= d < sqrt(82) passes the prefilter


def ca_sweep(a: int = 0, trailing: int = 2) -> dict:
    return turn_case([{"d": d} for d in CA_SWEEP], a, trailing)


BREAK_SWEEP = (ulps(2.5, -1), 2.5, ulps(2.5, 1))


def break_sweep(a: int = 0) -> dict:
    """C[a+2] on the x axis at |C[a+2] - N[a+3]| = v, O one further: H stays (1, 0, 0).  Above 2.5 a + 3 is no donor and no turn spans the break."""
    return turn_case([{"c2": (-v, 0.0, 0.0), "o2": (-v - 1.0, 0.0, 0.0)} for v in BREAK_SWEEP], a)


MIN_SWEEP = (ulps(0.5, -1), 0.5, ulps(0.5, 1))
MIN_WHICH = ("ON", "CH", "OH", "CN")


def min_variants() -> list:
    """(which distance, v, keyword arguments): O[a] or C[a] at exactly v from N = 0 or H = (1, 0, 0), along an axis through it; the other three stay above 0.5."""
    out = []
    for v in MIN_SWEEP:
        out.append(("ON", v, {"o": (-v, 0.0, 0.0), "c": (-v - 1.23, 0.0, 0.0)}))
        out.append(("CH", v, {"c": (1.0, v, 0.0), "o": (1.0, v + 1.23, 0.0)}))
        out.append(("OH", v, {"o": (1.0, v, 0.0), "c": (1.0, v + 1.23, 0.0)}))
        out.append(("CN", v, {"c": (-v, 0.0, 0.0), "o": (-v - 1.23, 0.0, 0.0)}))
    return out


def min_sweep(a: int = 0) -> dict:
    return turn_case([kw for _, _, kw in min_variants()], a)


# ---- 2: the bend probe ------------------------------------------------------------------------------------------------------------------------------------------------
def bend_atoms(t: float) -> list:
    """Five linked residues, CAs more than 9 A apart (no energies): CA[0] = (-20, 0, 0), CA[2] = 0, CA[4] = 20 (cos t, sin t, 0): kappa of residue 2 is t."""
    ca = [(-20.0, 0.0, 0.0), (-10.0, 30.0, 0.0), (0.0, 0.0, 0.0), (10.0, -30.0, 0.0), (20.0 * math.cos(t), 20.0 * math.sin(t), 0.0)]
    n = [(p[0] - 0.7, p[1], p[2] + 1.0) for p in ca]
    rows = []
    for r in range(5):
        c = up(n[r + 1]) if r < 4 else (ca[r][0] + 0.7, ca[r][1], ca[r][2] + 1.0)
        rows.append([n[r], ca[r], c, up(c, 1.2)])
    return rows


def bend_cos(t: float) -> float:
    rows = bend_atoms(t)
    return cos_kappa(rows[0][1], rows[2][1], rows[4][1])


@lru_cache(maxsize=None)
def bend_edge() -> tuple:
    """(t values, t0): t0 and its successor are adjacent doubles between which the restated cos kappa < cos 70 flips (from no bend to a bend)."""
    t0, _ = bisect_flip(lambda t: not bend_cos(t) < dc.COS70, math.radians(69.0), math.radians(71.0))
    return tuple(ulps(t0, k) for k in range(-6, 7)), t0


def bend_sweep(a: int = 0, trailing: int = 0) -> dict:
    frames = [{a + k: row for k, row in enumerate(bend_atoms(t))} for t in bend_edge()[0]]
    case = assemble(a + 5 + trailing, frames, {a + k: "A" for k in range(5)})
    case["probe"] = a
    return case


# ---- 3: the bridge probe ----------------------------------------------------------------------------------------------------------------------------------------------
def bridge_atoms(x1: float, x2: float) -> tuple:
    """(rows of i - 1, i, i + 1; rows of j - 1, j, j + 1).  O[i] <- H-N[j] on the line y = 0 (N[j] = 0, H[j] = (1, 0, 0), O[i] = (x1, 0, 0)) and O[j] <- H-N[i] on
    y = 5, reversed (N[i] = (0, 5, 0), H[i] = (-1, 5, 0), O[j] = (-x2, 5, 0)): the mirror image, so the second energy is the first's function of x2, bit for bit.
    The CAs of i and j are 2.4 A apart, those of the four neighbours are put by the caller (inert)."""
    o_i, c_i, n_i = (x1, 0.0, 0.0), (x1 + 1.23, 0.0, 0.0), (0.0, 5.0, 0.0)
    o_j, c_j, n_j = (-x2, 5.0, 0.0), (-x2 - 1.23, 5.0, 0.0), (0.0, 0.0, 0.0)
    left = [[(3.0, 6.0, 4.0), None, (1.0, 6.0, 0.0), (2.0, 6.0, 0.0)], [n_i, (0.0, 2.0, 1.0), c_i, o_i], [up(c_i), None, (9.0, 9.0, 4.0), (9.0, 9.0, 5.2)]]
    right = [[(-3.0, 1.0, 4.0), None, (-1.0, 1.0, 0.0), (-2.0, 1.0, 0.0)], [n_j, (0.0, 3.0, -1.0), c_j, o_j], [up(c_j), None, (-9.0, 9.0, 4.0), (-9.0, 9.0, 5.2)]]
    return left, right


def bridge_case(i: int, j: int, R: int) -> dict:
    """One bond at x = 3 and the other swept over the energy edge, then the other way round: 2 x the sweep's frames."""
    xs = energy_edge()[0]
    frames = []
    for x1, x2 in [(3.0, x) for x in xs] + [(x, 3.0) for x in xs]:
        left, right = bridge_atoms(x1, x2)
        fr = {}
        for at, rows in ((i, left), (j, right)):
            for k in (-1, 0, 1):
                fr[at + k] = list(rows[k + 1])
                if k:
                    fr[at + k][1] = inert_ca(at + k)
        frames.append(fr)
    chains = {i + k: "A" for k in (-1, 0, 1)}
    chains.update({j + k: "B" for k in (-1, 0, 1)})
    case = assemble(R, frames, chains)
    case["probe"] = (i, j)
    return case


BRIDGE_PLACES = ((1, 5, 8), (10, 300, 400), (63, 256, 400), (255, 64, 400), (64, 191, 400))

# ---- 4: the turn probe on the tile and stride boundaries ----------------------------------------------------------------------------------------------------------------
PLACES = {0: 2, 60: 0, 61: 0, 62: 3, 63: 3, 64: 3, 252: 0, 253: 0, 254: 3, 255: 3, 256: 3}     # a -> trailing pads; R = 64, 65, 256 and 257 among them


# ---- 5: the two best, and ties ------------------------------------------------------------------------------------------------------------------------------------------
SLOTS, DONOR, BEST_R = (5, 6, 70, 135), 200, 204      # acceptors in three LDS tiles (5 and 6 share one), the donor in a fourth
ORDER_X = (3.0, 3.5, 4.0)                             # three distinct energies, the lowest first


def best_frame(put: dict) -> dict:
    """put: {slot: (x, z)}: the acceptor at that index has O = (x, 0, z) and C = (x + 1.23, 0, z) against the donor's N = 0, H = (1, 0, 0); the other slots are
    padding in this frame.  Mirror images in z have bit-equal distances, so bit-equal energies."""
    fr = {DONOR - 1: [(-3.0, 1.0, 4.0), inert_ca(DONOR - 1), (-1.0, 1.0, 0.0), (-2.0, 1.0, 0.0)],
          DONOR: [(0.0, 0.0, 0.0), (0.0, -1.5, 0.0), (0.0, -3.0, 0.0), (0.0, -4.2, 0.0)]}
    for s in SLOTS:
        if s in put:
            x, z = put[s]
            fr[s] = [(5.0, -3.0, float(s)), (5.0, -1.5, 0.01 * s), (x + 1.23, 0.0, z), (x, 0.0, z)]
        else:
            fr[s] = pad(s)
    return fr


def best_plan() -> list:
    """(name, put, expected [entry 0, entry 1]) of every frame."""
    plan = []
    for perm in itertools.permutations(range(3)):
        put = {s: (ORDER_X[perm[k]], 0.0) for k, s in enumerate((5, 70, 135))}
        by_energy = [s for _, s in sorted((ORDER_X[perm[k]], s) for k, s in enumerate((5, 70, 135)))]
        plan.append(("order" + "".join(map(str, perm)), put, by_energy[:2]))
    plan += [("tie_same_tile", {5: (3.0, 1.0), 6: (3.0, -1.0), 70: (4.0, 0.0)}, [5, 6]),
             ("tie_same_tile_mirrored", {5: (3.0, -1.0), 6: (3.0, 1.0), 70: (4.0, 0.0)}, [5, 6]),
             ("tie_across_tiles", {5: (3.0, 1.0), 70: (3.0, -1.0), 135: (4.0, 0.0)}, [5, 70]),
             ("tie_for_second_then_better", {5: (3.5, 1.0), 70: (3.5, -1.0), 135: (3.0, 0.0)}, [135, 5]),
             ("tie_for_second_after_better", {5: (3.0, 0.0), 70: (3.5, 1.0), 135: (3.5, -1.0)}, [5, 70]),
             ("three_clamped", {5: (-0.25, 0.0), 70: (-0.3, 0.0), 135: (-0.4, 0.0)}, [5, 70]),
             ("four_clamped", {5: (-0.25, 0.0), 6: (-0.45, 0.0), 70: (-0.3, 0.0), 135: (-0.4, 0.0)}, [5, 6])]
    return plan


def best_case() -> dict:
    chains = {DONOR - 1: "A", DONOR: "A"}
    chains.update({s: pad_chain(s) for s in SLOTS})
    case = assemble(BEST_R, [best_frame(put) for _, put, _ in best_plan()], chains)
    case["probe"] = DONOR
    return case


# ---- 6: the crowded tile ----------------------------------------------------------------------------------------------------------------------------------------------
CROWD_R, CROWD_SEED = 130, 20


def crowded_case() -> dict:
    """One chain of 130 residues whose CAs lie in a ball of radius 4 A: every donor is near every acceptor, every mask of the sweep is full (bits 0 and 63
    included) and the last tile holds two acceptors.  N[r] = C[r-1] + a step of 1.3 A; C and O random within 1.5 A of the CA."""
    rng = np.random.default_rng(CROWD_SEED)
    unit = lambda n: (lambda v: v / np.linalg.norm(v, axis=1)[:, None])(rng.normal(size=(n, 3)))
    ca = unit(CROWD_R) * 4.0 * rng.uniform(0.0, 1.0, (CROWD_R, 1)) ** (1.0 / 3.0)
    xyz = np.zeros((1, CROWD_R, 4, 3))
    xyz[0, :, 1] = ca
    xyz[0, :, 2] = ca + unit(CROWD_R) * 1.5
    xyz[0, :, 3] = xyz[0, :, 2] + unit(CROWD_R) * 1.2
    xyz[0, 1:, 0] = xyz[0, :-1, 2] + unit(CROWD_R - 1) * 1.3
    xyz[0, 0, 0] = ca[0] + (1.0, 1.0, 0.0)
    case = dc.case_of([("ALA", "A", r + 1) for r in range(CROWD_R)], xyz)
    case["xyz"].setflags(write=False)
    return case


# ---- 7: features on the boundaries, real geometry ---------------------------------------------------------------------------------------------------------------------
UBQ_PADS = (35, 55, 63, 64, 227, 247)      # 1ubq's helix 23-34 (rows 22-33) or its first hairpin then straddles 63|64 or 255|256


def padded_ubq(k: int) -> dict:
    """k pads, then 1ubq; three frames, 1ubq rigidly tumbled about its own centroid in the last two (the pads stay)."""
    ubq = dc.pdb_case("1ubq.pdb")
    n = len(ubq["res"])
    flat = ubq["xyz"][0].reshape(4 * n, 3)
    moved = ts.tumble(flat, 3, 5)
    res = [("ALA", pad_chain(r), r + 1) for r in range(k)] + [(resn, "A", resi) for resn, _, resi in ubq["res"]]
    xyz = np.zeros((3, k + n, 4, 3))
    for f, body in enumerate((flat, moved[1], moved[2])):
        for r in range(k):
            xyz[f, r] = pad(r)
        xyz[f, k:] = body.reshape(n, 4, 3)
    case = dc.case_of(res, xyz)
    case["xyz"].setflags(write=False)
    case["string"] = "-" * k + dc.UBQ_STRING
    return case


LONG_R = 300


def long_helix(kind: str) -> dict:
    case = dc.helix(kind, LONG_R)
    case["xyz"].setflags(write=False)
    case["string"] = "-" + {"alpha": "H", "310": "G", "pi": "I"}[kind] * (LONG_R - 2) + "-"
    return case


SPLIT_AT = (64, 256)
SPLIT_STRING = "-" + "H" * 62 + "--" + "H" * 190 + "--" + "H" * 42 + "-"


def split_helix(proline: int | None = None) -> dict:
    """The alpha helix of 300 residues as three chains (a chain start on residues 64 and 256), optionally with a proline (no amide hydrogen)."""
    base = dc.helix("alpha", LONG_R)
    res = [("PRO" if r == proline else "ALA", "ABC"[sum(r >= s for s in SPLIT_AT)], r + 1) for r in range(LONG_R)]
    case = dc.case_of(res, base["xyz"])
    case["xyz"].setflags(write=False)
    assert np.flatnonzero(case["flags"] & dc.CHAIN_START).tolist() == [0, *SPLIT_AT]
    if proline is None:
        case["string"] = SPLIT_STRING
    return case


PROLINE_AT = 130


# ---- every case, by name ------------------------------------------------------------------------------------------------------------------------------------------------
BUILDERS = {"energy": energy_sweep, "ca": ca_sweep, "ca_a62": lambda: ca_sweep(62, 3), "break": break_sweep, "min": min_sweep, "bend": bend_sweep,
            "bend_a254": lambda: bend_sweep(254, 2), "best": best_case, "crowded": crowded_case, "split": split_helix, "split_pro": lambda: split_helix(PROLINE_AT)}
BUILDERS.update({f"bridge_{i}_{j}": (lambda i=i, j=j, R=R: bridge_case(i, j, R)) for i, j, R in BRIDGE_PLACES})
BUILDERS.update({f"place_{a}": (lambda a=a, t=t: energy_sweep(a, t)) for a, t in PLACES.items() if a})
BUILDERS.update({f"ubq_pad{k}": (lambda k=k: padded_ubq(k)) for k in UBQ_PADS})
BUILDERS.update({f"long_{kind}": (lambda kind=kind: long_helix(kind)) for kind in dc.HELIX_ANGLES})
NAMES = sorted(BUILDERS)
MARGIN_CASES = tuple(n for n in NAMES if n.startswith(("ubq_pad", "long_", "split")))     # real geometry on launch boundaries: they keep dssp_cases' margins
SWEEPS = tuple(n for n in NAMES if n in ("energy", "ca", "ca_a62", "break", "min", "bend", "bend_a254", "best") or n.startswith(("bridge_", "place_")))   # several frames


@lru_cache(maxsize=None)
def case(name: str) -> dict:
    c = BUILDERS[name]()
    if name in MARGIN_CASES:
        assert dc.clear(c["xyz"], c["flags"]), (name, dc.margins(c["xyz"], c["flags"]))
    return c


@lru_cache(maxsize=None)
def want(name: str) -> dict:
    """The restated expectation of a case, computed once and left unchanged."""
    w = expected(case(name))
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w
