"""Cases and references for the covariance, the DCCM and the projection of an ensemble's motions (arp_covariance, arp_project: cov.inl behind rmsf.inl, the host
half in cov.cpp).  No product imports: tests/test_cov_host.py checks arp_covariance_host, arp_project_host, the input checks and every case's reach on the CPU,
tests/test_cov_gpu.py runs the cases on the device.  Built on rmsf_cases (the superposition, its bounds, the layouts) and rmsd_cases.

Reference: numpy f64.  rmsf_cases.reference gives the superposed measured atoms Y and their mean; D[F, 3m] = Y - mean with the coordinate index a = 3 i + k;
cov = D^T D / F;  t_ij = (1 / F) sum_f sum_k d_f,(i,k) d_f,(j,k), v_i = t_ii, dccm = clamp(t_ij / sqrt(v_i v_j), -1, 1), diagonal 1, 0 where a v is 0.

Bounds (derived, not tuned).  tau_f,i = rmsf_cases' bound on |dY_f,i| (its `aligned` bound without the term of absolute coordinates) plus its bound on the mean
(likewise); a vector's bound holds for each of its components, so tau_a = tau_i for a = (i, k).  With d the reference's deviations:
  cov   |dcov_ab| <= (1 / F) sum_f (|d_a| tau_b + tau_a |d_b| + tau_a tau_b)  +  (F + 4) eps (1 / F) sum_f |d_a| |d_b|
        the first sum is the product rule on d + dd; the second holds for ANY order of summing F products (the MFMA's and the slabs' included): F - 1
        additions and one product rounding each, one division by F, and the two roundings of d = Y - mean.
  t     the same over the 3 F terms (frame, component) of atom pair (i, j): (3 F + 4) eps in the second term.  dv_i = dt_ii.
  dccm  dt_ij / sqrt(v_i v_j) + |c| (dv_i / (2 v_i) + dv_j / (2 v_j)) + 2^-23     (first order in dv / v, which the reach checks hold below 10^-3; the
        last term is the one rounding to f32, 2^-24 for |c| <= 1, and the f64 division and square root)
  proj  sum_a tau_a |V_ja| + (3 m + 2) eps sum_a |d_a| |V_ja|, where arp_project's tau_a is the term of absolute coordinates, 4 eps max |coordinate| per
        atom, because it forms R p + t - mean from absolute coordinates (rmsf_cases: `big`); its transforms and mean are inputs, taken as exact.  The
        reference evaluates the same formula in numpy's long double where that is wider than f64 (x86: 64-bit mantissa); where it is not, the reference
        carries the same term and the bound holds it twice.
An iterated call multiplies tau by rmsf_cases' (rounds + 1) -- unproven there and here, named `scale`.  Where two computed results are compared (the device
against the host yardstick fed by arp_rmsf_host) the bound is the sum of both sides' bounds against numpy.
The fits with gap 0 (collinear, n <= 2) have no bound (tau is infinite): they are checked on invariants only, as in rmsf_cases.

The kernels' constants (cov.inl, table_dev.h), which the shapes below straddle:
  STEP        = 4     m_pad is m rounded up to it (the pack of rmsd.inl); also the contraction rows of one MFMA (16 x 16 x 4)
  WAVE        = 16    rows and columns of a wave's tile
  TILE        = 32    rows and columns of a workgroup's tile: 2 x 2 waves.  Rows are the 3 m_pad coordinates (cov) or the m_pad atoms (dccm)
  CHUNK       = 16    contraction rows staged through LDS per step; a frame is 1 row (cov) or 3 (dccm)
  SLAB_MIN    = 64    frames of the shortest slab
  GRID_TARGET = 1024  workgroups wanted: slab_frames = max(SLAB_MIN, ceil(F / ceil(GRID_TARGET / tiles)) rounded up to CHUNK), tiles = T (T + 1) / 2
  PROJ_TILE   = 16    frames and modes of a workgroup of k_project;  PROJ_ATOMS = 16 atoms per step of its loop
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import rmsd_cases as rc
import rmsf_cases as fc
import trajectory_shapes as ts

STEP, WAVE, TILE, CHUNK, SLAB_MIN, GRID_TARGET, PROJ_TILE, PROJ_ATOMS = 4, 16, 32, 16, 64, 1024, 16, 16
EPS = rc.EPS
MAX_F, MAX_ATOMS = 300, 260
MIN_SIGNAL = 1e3        # v_i / its bound of every case compared on dccm
KINDS = fc.KINDS
WIDE = bool(np.finfo(np.longdouble).eps < 2.0 ** -60)   # numpy's long double is wider than f64

ATOMS = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
FRAMES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 300]
MIXED = [(33, 20, "disjoint", 65), (65, 64, "overlap", 31), (130, 5, "contains", 130), (300, 17, "contains", 260), (4, 33, "disjoint", 3), (200, 16, "overlap", 17)]


def pad(m: int) -> int:
    return -(-m // STEP) * STEP


def slab_plan(F: int, L: int) -> tuple:
    """(slab_frames, slabs) of a Gram over L rows and columns: table_dev.h cov_plan restated."""
    T = -(-L // TILE)
    want = -(-GRID_TARGET // (T * (T + 1) // 2))
    slab = max(SLAB_MIN, -(-(-(-F // want)) // CHUNK) * CHUNK)
    return slab, -(-F // slab)


def shapes() -> list:
    """(F, n, kind, m): every m at F = 5 and F = 65 and every F at m = 5 and m = 33, measured on the fit atoms; then the measured sets of their own."""
    out = [(F, n, "same", n) for n in ATOMS for F in (5, 65)] + [(F, n, "same", n) for F in FRAMES for n in (5, 33)]
    return sorted(set(out)) + MIXED


def cov_only(case: tuple) -> bool:
    """F = 1: nothing moves, every v is exactly 0 -- cov is compared (it is exactly 0), the dccm is checked on its own definition (0.0f off the diagonal)."""
    return case[0] == 1


def check_shape_reach() -> dict:
    S = shapes()
    Fs, ms = {s[0] for s in S}, {s[3] for s in S}
    assert max(Fs) <= MAX_F and max(ms | {s[1] for s in S}) <= MAX_ATOMS
    assert {1, 2, 3, 4, 5} <= ms and {1, 2, 3, 4, 5} <= Fs                                      # the 4-step pad; the K step of the MFMA
    for edge in (WAVE, TILE, 2 * TILE):
        assert {edge - 1, edge, edge + 1} <= ms, edge                                           # the dccm end: rows are atoms
    Ls = {3 * pad(m) for m in ms}
    assert any(L < WAVE for L in Ls) and any(WAVE < L < TILE for L in Ls) and {max(L for L in Ls if L < TILE), min(L for L in Ls if L > TILE)} == {24, 36}
    assert any(L % TILE == 0 and L >= 2 * TILE for L in Ls) and any(L > 2 * TILE and L % TILE for L in Ls)   # the cov end: whole tiles; a partial last one
    assert any(pad(m) > 2 * TILE and pad(m) % TILE for m in ms)                                 # the dccm end: at least two tiles and a partial last one
    for edge in (CHUNK, SLAB_MIN, 2 * SLAB_MIN):
        assert {edge - 1, edge, edge + 1} <= Fs, edge                                           # a chunk, one slab and two slabs from both sides
    plans = {(s[0], s[3]): (slab_plan(s[0], 3 * pad(s[3])), slab_plan(s[0], pad(s[3]))) for s in S}
    assert any(p[0][1] > 2 and F % p[0][0] for (F, m), p in plans.items())                      # more than two slabs and a partial last one
    assert any(p[0][0] > SLAB_MIN and p[0][1] > 1 for p in plans.values())                      # slabs longer than the shortest (the grid target binds)
    assert any(p[0] != p[1] for p in plans.values())                                            # the two ends of one call with different plans
    assert {s[2] for s in S} == set(KINDS)
    # k_project (every shape is projected): a workgroup's frames and modes, and the atoms of a step of its loop, from both sides and at whole multiples
    for edge in (PROJ_TILE, 2 * PROJ_TILE, 4 * PROJ_TILE):
        assert {edge - 1, edge, edge + 1} <= Fs, ("frames of k_project", edge)
    for edge in (PROJ_ATOMS, 2 * PROJ_ATOMS, 4 * PROJ_ATOMS):
        assert {edge - 1, edge, edge + 1} <= ms, ("atoms of k_project", edge)
    assert any(m < PROJ_ATOMS for m in ms) and any(F < PROJ_TILE for F in Fs) and any(m % PROJ_ATOMS > 1 and m > 2 * PROJ_ATOMS for m in ms)
    assert {PROJ_TILE - 1, PROJ_TILE, PROJ_TILE + 1} <= set(MODE_COUNTS) and 1 in MODE_COUNTS
    assert any(3 * m > 2 * PROJ_TILE and 3 * m % PROJ_TILE for m in ms) and any(3 * m % PROJ_TILE == 0 for m in ms)   # k = 3 m: several mode tiles, partial and whole
    through, invariants = [], []
    for s in S:
        ref = reference(s)
        if s[1] <= 2:
            assert ref["base"]["gap_ratio"] <= 1e-9, (s, ref["base"]["gap_ratio"])
            invariants.append(s)
            continue
        assert ref["base"]["gap_ratio"] >= fc.MIN_GAP, (s, ref["base"]["gap_ratio"])
        through.append(s)
        if cov_only(s):
            assert (ref["cov"] == 0).all() and (ref["v"] == 0).all(), s
        else:
            assert (ref["v"] >= MIN_SIGNAL * ref["v_bound"]).all(), (s, float((ref["v"] / ref["v_bound"]).min()))
    assert {s[1] for s in invariants} == {1, 2}
    return {"through_R": through, "invariants_only": invariants}


# ---- reference and bounds ------------------------------------------------------------------------------------------------------------------------------------
def deviations(base: dict) -> np.ndarray:
    """D [F, 3m] of an rmsf_cases.reference result: the superposed measured atoms minus their mean, a = 3 i + k."""
    Y = base["aligned"] - base["c_t"]
    return (Y - Y.mean(0)).reshape(len(Y), -1)


def tau_of(base: dict) -> np.ndarray:
    """tau [F, m] of the module docstring, the iterated factor included."""
    return ((base["bound"]["aligned"] - base["big"]) + (base["bound"]["mean"] - base["big"])[None]) * base["scale"]


def dccm_of(t: np.ndarray) -> np.ndarray:
    v = np.diag(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.clip(t / np.sqrt(np.outer(v, v)), -1.0, 1.0)
    c[np.outer(v, v) == 0] = 0.0
    np.fill_diagonal(c, 1.0)
    return c


def second_moments(D: np.ndarray, tau: np.ndarray) -> dict:
    """cov, t, v, dccm of D [F, 3m] and their bounds for deviations known to tau [F, m] per atom."""
    F, L = D.shape
    m = L // 3
    A, T3 = np.abs(D), np.repeat(tau, 3, axis=1)
    cov = D.T @ D / F
    AA = A.T @ A / F
    with np.errstate(invalid="ignore"):
        cov_bound = (A.T @ T3 + T3.T @ A + T3.T @ T3) / F + (F + 4) * EPS * AA
    fold = lambda M: M.reshape(m, 3, m, 3)[:, [0, 1, 2], :, [0, 1, 2]].sum(0)      # sum over k of the (i, k), (j, k) entries
    t = fold(cov)
    t_bound = fold(cov_bound) + 2 * F * EPS * fold(AA)                             # (3 F + 4) eps in all
    v, v_bound = np.diag(t).copy(), np.diag(t_bound).copy()
    c = dccm_of(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.sqrt(np.outer(v, v))
        rel = v_bound / (2.0 * v)
        dccm_bound = t_bound / root + np.abs(c) * (rel[:, None] + rel[None, :]) + 2.0 ** -23
    dccm_bound[~np.isfinite(dccm_bound)] = np.inf
    np.fill_diagonal(dccm_bound, 0.0)
    return {"cov": cov, "cov_bound": cov_bound, "t": t, "t_bound": t_bound, "v": v, "v_bound": v_bound, "dccm": c, "dccm_bound": dccm_bound}


def reference_of(X, XM=None, ref=0, max_rounds: int = 1, tol: float = 0.0, extra_tau: float = 0.0) -> dict:
    """Everything above from the fit atoms X [F, n, 3] and the measured atoms XM (None: X); `base`: rmsf_cases.reference's result; `D`, `tau`."""
    base = fc.reference(X, XM, ref, max_rounds, tol)
    D, tau = deviations(base), tau_of(base) + extra_tau
    return dict(second_moments(D, tau), base=base, D=D, tau=tau)


@lru_cache(maxsize=None)
def _reference(case: tuple):
    c = fc.shape_case(*case)
    return reference_of(c["frames"][:, c["sel"]], None if c["msel"] is None else c["frames"][:, c["msel"]])


def reference(case: tuple) -> dict:
    """The reference of one shape, computed once and shared; treat it as read-only."""
    return _reference(tuple(case))


def assert_within(got: dict, ref: dict, what="", keys=("covariance", "dccm"), slack: dict | None = None) -> float:
    """got["covariance"] / got["dccm"] within the bounds of ref (plus slack[key], another side's bound); returns the largest error / bound ratio."""
    worst = 0.0
    for key in keys:
        if key not in got:
            continue
        want, bound = (ref["cov"], ref["cov_bound"]) if key == "covariance" else (ref["dccm"], ref["dccm_bound"])
        if slack and key in slack:
            bound = bound + slack[key]
        err = np.abs(np.asarray(got[key], np.float64) - want)
        bad = np.argwhere(~(err <= bound))
        if len(bad):
            k = tuple(bad[0])
            raise AssertionError(f"{what} {key}: {len(bad)} entries outside the bound, first {list(k)}: error {err[k]:.3e}, bound {bound[k]:.3e}")
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where((bound > 0) & np.isfinite(bound), err / bound, 0.0)
        worst = max(worst, float(ratio.max()))
    return worst


def check_matrices(got: dict, m: int, what=""):
    """What holds of any result: the types, the shapes, symmetric bits, the dccm's diagonal and range."""
    if "covariance" in got:
        c = got["covariance"]
        assert c.dtype == np.float64 and c.shape == (3 * m, 3 * m) and c.tobytes() == np.ascontiguousarray(c.T).tobytes(), (what, "cov symmetric")
        assert np.isfinite(c).all() and (np.diag(c) >= 0).all(), what
    if "dccm" in got:
        d = got["dccm"]
        assert d.dtype == np.float32 and d.shape == (m, m) and d.tobytes() == np.ascontiguousarray(d.T).tobytes(), (what, "dccm symmetric")
        assert (np.diag(d) == np.float32(1.0)).all() and (np.abs(d) <= 1.0).all(), what


# ---- projection ----------------------------------------------------------------------------------------------------------------------------------------------
def random_modes(m: int, k: int, seed: int = 5) -> np.ndarray:
    """k rows over the 3 m coordinates, neither orthogonal nor unit."""
    return np.random.default_rng(seed + 131 * m + k).normal(size=(k, 3 * m))


def projection(P: np.ndarray, transforms, mean: np.ndarray, modes: np.ndarray, big: float, tau=None) -> dict:
    """proj [F, k] of absolute measured coordinates P [F, m, 3], transforms [F, 12] (None: identity), mean [m, 3] and modes [k, 3m], and its bound; tau
    [F, m]: what the deviations are known to beyond the term of absolute coordinates `big`."""
    wide = np.longdouble if WIDE else np.float64
    F, m = P.shape[:2]
    Pw = np.asarray(P, wide)
    if transforms is None:
        Y = Pw
    else:
        tr = np.asarray(transforms, wide)
        Y = np.einsum("fab,fib->fia", tr[:, :9].reshape(F, 3, 3), Pw) + tr[:, None, 9:]
    D = (Y - np.asarray(mean, wide)).reshape(F, 3 * m)
    proj = (D @ np.asarray(modes, wide).T).astype(np.float64)
    per_atom = (0.0 if tau is None else tau) + big * (1.0 if WIDE else 2.0)
    V = np.abs(np.asarray(modes, np.float64))
    bound = np.repeat(np.broadcast_to(per_atom, (F, m)), 3, axis=1) @ V.T + (3 * m + 2) * EPS * (np.abs(D).astype(np.float64) @ V.T)
    return {"proj": proj, "bound": bound, "D": D.astype(np.float64)}


def ratio_within(got: np.ndarray, want: np.ndarray, bound: np.ndarray, what="") -> float:
    err = np.abs(np.asarray(got, np.float64) - want)
    bad = np.argwhere(~(err <= bound))
    if len(bad):
        k = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} entries outside the bound, first {list(k)}: error {err[k]:.3e}, bound {bound[k]:.3e}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, 0.0).max()) if err.size else 0.0


MODE_COUNTS = (1, 15, 16, 17)    # and 3 m: one below, at and one above a workgroup's modes


def mode_counts(m: int) -> list:
    """The k every shape is projected at: 1, 15, 16, 17 where 3 m allows, and 3 m."""
    return sorted({min(k, 3 * m) for k in MODE_COUNTS} | {3 * m})


# ---- the closed-form fixture -----------------------------------------------------------------------------------------------------------------------------------
SCAFFOLD = 20
S_SEQ = np.array([1.0, 1.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0])     # sum s = sum c = sum s c = 0;  mean s^2 = 1/2, mean c^2 = 3/2
C_SEQ = np.array([1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 0.0, 0.0])
A_AMP = np.array([1.0, -2.0, 0.5, 0.0, 0.0, 0.0, -0.25, 0.0])    # every measured atom moves along x or along y, none along both, none not at all
B_AMP = np.array([0.0, 0.0, 0.0, 1.0, -0.5, 2.0, 0.0, -4.0])


@lru_cache(maxsize=None)
def closed_form() -> dict:
    """A rigid scaffold of 20 fit atoms, the same in every frame, and 8 measured atoms disjoint from it at p_i + a_i s_f e_x + b_i c_f e_y in the scaffold's
    frame; every frame tumbled and shifted as a whole.  Fitted to the untumbled scaffold (`ref_xyz`), cov is a_i a_j mean(s^2) on the xx block,
    b_i b_j mean(c^2) on the yy block and 0 elsewhere, and dccm is +1, -1 or 0 -- no numerical reference is needed for the expected values."""
    rng = np.random.default_rng(2024)
    m, F = len(A_AMP), len(S_SEQ)
    N = SCAFFOLD + m
    rest = rng.normal(scale=8.0, size=(N, 3))
    sel = np.sort(rng.permutation(N)[:SCAFFOLD]).astype("<u4")
    msel = np.setdiff1d(np.arange(N), sel).astype("<u4")
    frames = np.empty((F, N, 3))
    for f in range(F):
        local = rest.copy()
        local[msel, 0] += A_AMP * S_SEQ[f]
        local[msel, 1] += B_AMP * C_SEQ[f]
        frames[f] = local @ ts.random_rotation(rng).T + rng.normal(scale=30.0, size=3)
    cov = np.zeros((3 * m, 3 * m))
    cov[0::3, 0::3] = np.outer(A_AMP, A_AMP) * (S_SEQ ** 2).mean()
    cov[1::3, 1::3] = np.outer(B_AMP, B_AMP) * (C_SEQ ** 2).mean()
    t = cov[0::3, 0::3] + cov[1::3, 1::3]
    dccm = np.sign(t)
    np.fill_diagonal(dccm, 1.0)
    D = np.zeros((F, m, 3))
    D[:, :, 0], D[:, :, 1] = np.outer(S_SEQ, A_AMP), np.outer(C_SEQ, B_AMP)
    frames.setflags(write=False)
    return {"N": N, "sel": sel, "msel": msel, "frames": frames, "ref_xyz": rest, "cov": cov, "dccm": dccm, "D": D.reshape(F, -1)}


def closed_form_bounds() -> dict:
    """The bounds of the module docstring around the closed form: tau from rmsf_cases for this fit, plus the term of absolute coordinates, to which the
    tumbled frames themselves hold the closed form (their coordinates are rounded where they stand)."""
    fx = closed_form()
    base = fc.reference(fx["frames"][:, fx["sel"]], fx["frames"][:, fx["msel"]], ref=fx["ref_xyz"][fx["sel"]])
    out = second_moments(fx["D"], tau_of(base) + base["big"])
    assert np.array_equal(out["dccm"], fx["dccm"]) and np.abs(out["cov"] - fx["cov"]).max() == 0.0      # (the closed form is exact in f64)
    return dict(out, base=base)


def closed_form_projection() -> dict:
    """The closed-form fixture projected on the unit modes e_a: proj[f][a] is the deviation d_f,a itself, known exactly.  Its bound per coordinate: tau of the
    superposition that supplies the transforms and the mean, the term of absolute coordinates once for the tumbled frames (they hold the closed form to the
    rounding of where they stand), once for the transforms and the mean as outputs of that superposition, and once for R p + t - mean in arp_project; the
    summation term is (3 m + 2) eps |d_a|, a sum with one non-zero term."""
    fx, b = closed_form(), closed_form_bounds()
    F, L = fx["D"].shape
    per = np.repeat(tau_of(b["base"]) + 3.0 * b["base"]["big"], 3, axis=1)
    return {"modes": np.eye(L), "proj": fx["D"], "bound": per + (L + 2) * EPS * np.abs(fx["D"])}


def check_closed_form_reach():
    fx, b = closed_form(), closed_form_bounds()
    assert S_SEQ.sum() == C_SEQ.sum() == (S_SEQ * C_SEQ).sum() == 0 and not set(fx["sel"].tolist()) & set(fx["msel"].tolist())
    assert ((A_AMP != 0) ^ (B_AMP != 0)).all() and {-1.0, 0.0, 1.0} == set(np.unique(fx["dccm"]))
    assert b["base"]["gap_ratio"] >= fc.MIN_GAP and (b["v"] >= MIN_SIGNAL * b["v_bound"]).all()
    assert b["cov_bound"].max() < 1e-9 and b["dccm_bound"].max() < 1e-6
    # numpy's own superposition finds the closed form within those bounds
    ref = reference_of(fx["frames"][:, fx["sel"]], fx["frames"][:, fx["msel"]], ref=fx["ref_xyz"][fx["sel"]])
    assert (np.abs(ref["cov"] - fx["cov"]) <= b["cov_bound"]).all() and (np.abs(ref["dccm"] - fx["dccm"]) <= b["dccm_bound"]).all()


# ---- one rigid shape tumbled: nothing moves ----------------------------------------------------------------------------------------------------------------------
def rigid_case() -> np.ndarray:
    return rc.degenerate_cases()["tumble"]


def rigid_bound() -> dict:
    """cov of rigid copies is 0 to the bound with the term of absolute coordinates in tau (rmsf_cases.assert_rigid: the copies are rigid only to the rounding
    of their own coordinates); every v lies below its bound, so the dccm means nothing and is not compared."""
    X = rigid_case()
    base = fc.reference(X)
    out = second_moments(deviations(base), tau_of(base) + base["big"])
    assert (out["v"] <= out["v_bound"]).all()
    return out


# ---- PCA -------------------------------------------------------------------------------------------------------------------------------------------------------
def fix_signs(modes: np.ndarray) -> np.ndarray:
    """Each row with its largest-magnitude component positive, the lowest index on ties."""
    out = np.array(modes, np.float64)
    for row in out:
        j = int(np.argmax(np.abs(row)))
        if row[j] < 0:
            row *= -1.0
    return out


def capacity_bytes(F: int, n: int, m: int, own: bool, cov: bool, dccm: bool) -> int:
    """What arp_covariance checks against "rmsd_cap_bytes": arp_rmsf's resident state, the deviations, the outputs at their padded sizes, the larger of the
    two ends' slab partials."""
    n_pad, m_pad = pad(n), pad(m)
    part = lambda L: slab_plan(F, L)[1] * (-(-L // TILE) * (-(-L // TILE) + 1) // 2) * TILE * TILE
    need = F * 3 * n_pad * 8 + F * 8 + (F * 3 * m_pad * 8 if own else 0) + F * 3 * m_pad * 8
    need += (9 * m_pad * m_pad * 8 if cov else 0) + (m_pad * m_pad * 4 if dccm else 0)
    return need + 8 * max(part(3 * m_pad) if cov else 0, part(m_pad) if dccm else 0)
