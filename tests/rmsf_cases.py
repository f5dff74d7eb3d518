"""Cases and references for RMSF and the mean structure (arp_rmsf: rmsf.inl + the host half in rmsf.cpp).  No product imports: tests/test_rmsf_host.py checks
arp_rmsf_host, the input checks and every case's reach on the CPU, tests/test_rmsf_gpu.py runs the cases on the device.

Reference: numpy f64.  Centre every frame on the centroid of its fit atoms (in two steps: the mean, then the mean of what is left, so that a frame 10^5 A from
the origin is centred to the rounding of its centred coordinates), S_f = X_f^T T, the SVD route of rmsd_cases.top_eigenvalue with R = V diag(1, 1, d) U^T,
Y = R x, the mean over the frames, and -- iterated -- the mean as the next target.

Tolerance (derived, not tuned; the constant 64 is rmsd_cases'): with Gs_f = G_f + G_T and gap_f = lambda_1 - lambda_2 of K(S_f) = 2 (s_2 + d s_3), the entries
of K err by at most 64 eps Gs_f, so the top eigenvector turns by at most u_f = 2 . 64 eps Gs_f / gap_f (Davis-Kahan) and
    |dY_f,i| <= 2 u_f |x_f,i| + 8 eps |x_f,i| =: tau_f,i        (absolute coordinates -- aligned, mean, t -- add 4 eps max |coordinate|)
  mean        mean_f tau_f,i + F eps max_f |Y_f,i|
  rmsf        2 max_f tau_f,i + 2^-23 rmsf            (the triangle inequality of an L2 norm, and the one rounding to f32)
  frame_rmsd  2 max_i tau_f,i + 2^-23 r
  R, t        entries of R: 2 u_f + 8 eps (tau of a unit vector); t = c_T - R c_f: (2 u_f + 8 eps) |c_f| + 4 eps max |coordinate|
An iterated call is held to (rounds + 1) x the bound of its last round (every round adds one round's error to its target; not proven, the largest observed
ratio is recorded in profiles/ and DESIGN.md section 3.21).  The gap is a condition on the inputs: every case compared through R has gap_f >= 10^-2 Gs_f,
asserted by the reach checks, which also list the cases that are compared on invariants only (gap 0: collinear fit atoms, n <= 2).

The kernels' constants (rmsf.inl), which the shapes below straddle:
  LANES      = 64   lanes of a frame in the fit and in frame_rmsd: one wave; lane l sums the atoms l, l + 64, ..
  FIT_FRAMES = 4    frames (waves) of a workgroup of those kernels
  TILE       = 64   atoms of a tile of the sweeps over frames (mean, deviation)
  SLAB       = 32   frames of a slab of those sweeps; the slabs are summed in their order afterwards
  FINISH     = 64   items of a workgroup of the kernels that sum the slabs: the 3 n_pad (component, atom) pairs of the mean, the m atoms of the deviations
  FINISH_LANES = 4  waves of such a workgroup: wave j sums the slabs j, j + 4, .. of its items, the four meet in a fixed tree
  STEP       = 4    n_pad and m_pad are n and m rounded up to it (the pack of rmsd.inl)
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import rmsd_cases as rc
import trajectory_shapes as ts

LANES, FIT_FRAMES, TILE, SLAB, FINISH, FINISH_LANES, STEP = 64, 4, 64, 32, 64, 4, 4
EPS = rc.EPS
MIN_GAP = 1e-2          # gap_f / Gs_f of every case that is compared through R
MAX_F, MAX_ATOMS = 130, 602

FRAMES = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 70, 127, 128, 129, 130]
ATOMS = [1, 2, 3, 4, 5, 20, 21, 63, 64, 65, 602]
KINDS = ("same", "disjoint", "overlap", "contains")   # msel: none given (= sel), no atom shared with sel, some shared, every atom of sel and more
MIXED = [(33, 64, "disjoint", 65), (5, 65, "overlap", 63), (70, 5, "contains", 257), (3, 255, "disjoint", 1), (130, 17, "contains", 64), (2, 4, "overlap", 256),
         (65, 63, "disjoint", 255), (4, 3, "contains", 602)]


def shapes() -> list:
    """(F, n, kind, m): every F at n = 5 and n = 65, every n at F = 5 and F = 33, measured on the fit atoms; then the measured sets of their own."""
    out = [(F, n, "same", n) for F in FRAMES for n in (5, 65)] + [(F, n, "same", n) for n in ATOMS for F in (5, 33)]
    return sorted(set(out)) + MIXED


def check_shape_reach():
    S = shapes()
    Fs, ns, ms = {s[0] for s in S}, {s[1] for s in S}, {s[3] for s in S}
    assert max(Fs) <= MAX_F and max(ns | ms) <= MAX_ATOMS
    assert {1, 2} <= Fs and {1, 2, 3, 4, 5} <= ns
    for edge in (FIT_FRAMES, SLAB, 2 * SLAB):
        assert {edge - 1, edge, edge + 1} <= Fs, edge                      # a workgroup of the fit, one slab and two slabs from both sides
    assert any(F > 2 * SLAB and F % SLAB for F in Fs) and any(-(-F // SLAB) >= 5 for F in Fs)   # more than two slabs with a partial last one
    for edge in (STEP, LANES, TILE, FINISH):
        assert {edge - 1, edge, edge + 1} <= ns and {edge - 1, edge, edge + 1} <= ms, edge
    assert any(n > LANES for n in ns)                                            # a lane of the fit with more than one atom
    pad = lambda n: -(-n // STEP) * STEP
    assert any(3 * pad(n) < FINISH for n in ns) and {3 * pad(n) // FINISH for n in (20, 21)} == {0, 1} and any(3 * pad(n) % FINISH == 0 for n in ns) and \
        any(3 * pad(n) > 2 * FINISH and 3 * pad(n) % FINISH for n in ns)        # the mean's items: less than a workgroup, whole workgroups, a partial last one
    edge = FINISH_LANES * SLAB                                                   # four slabs: every wave of a finish workgroup has one; a fifth goes to wave 0 again
    assert {edge - 1, edge, edge + 1} <= Fs
    assert {s[2] for s in S} == set(KINDS)
    for F, n, kind, m in MIXED:
        c = shape_case(F, n, kind, m)
        sel, msel = set(c["sel"].tolist()), set(c["msel"].tolist())
        assert len(sel) == n and len(msel) == m and m != n
        assert {"disjoint": not sel & msel, "overlap": bool(sel & msel) and bool(sel - msel) and bool(msel - sel), "contains": sel < msel}[kind], (F, n, kind, m)
    through, invariants = [], []
    for s in S:
        c = shape_case(*s)
        ref = reference(c["frames"][:, c["sel"]], None if c["msel"] is None else c["frames"][:, c["msel"]])
        (through if s[1] > 2 else invariants).append(s)
        if s[1] > 2:
            assert ref["gap_ratio"] >= MIN_GAP, (s, ref["gap_ratio"])
        else:
            assert ref["gap_ratio"] <= 1e-9, (s, ref["gap_ratio"])               # n <= 2: the top eigenvalue of K is double
    assert {s[1] for s in invariants} == {1, 2} and len(through) + len(invariants) == len(S)
    return {"through_R": through, "invariants_only": invariants}


# ---- the shapes' data ----------------------------------------------------------------------------------------------------------------------------------------
def layout(n: int, kind: str, m: int) -> tuple:
    """(N, sel, msel or None): where the fit and the measured atoms sit among the N atoms of the topology; the atoms of neither are decoys the pack skips."""
    if kind == "same":
        N = n + 2
        return N, np.delete(np.arange(N), [0, N // 2]).astype("<u4"), None
    if kind == "disjoint":
        N = n + m + 1
        mixed = np.random.default_rng(n + 1000 * m).permutation(np.delete(np.arange(N), [N // 2]))   # interleaved: neither set is a contiguous run
        return N, np.sort(mixed[:n]).astype("<u4"), np.sort(mixed[n:]).astype("<u4")
    if kind == "overlap":
        N = n + m
        return N, np.arange(n, dtype="<u4"), np.arange(n // 2, n // 2 + m, dtype="<u4")
    if kind == "contains":
        assert m > n
        return m + 1, ((np.arange(n) * m) // n).astype("<u4"), np.arange(m, dtype="<u4")
    raise ValueError(kind)


def ensemble(base: np.ndarray, F: int, seed: int, sigma: float, shift: float = 50.0) -> np.ndarray:
    """[F, N, 3]: base + N(0, sigma) per atom and frame, then a seeded rotation and a translation of N(0, shift) per frame."""
    rng = np.random.default_rng(seed)
    return np.stack([(base + rng.normal(scale=sigma, size=base.shape)) @ ts.random_rotation(rng).T + rng.normal(scale=shift, size=3) for _ in range(F)])


@lru_cache(maxsize=None)
def _shape_case(F: int, n: int, kind: str, m: int):
    N, sel, msel = layout(n, kind, m)
    base = np.random.default_rng(7919 * n + m).normal(scale=rc.SIGMA, size=(N, 3))
    frames = ensemble(base, F, 1000003 * F + 31 * n + m, 1.0)
    frames.setflags(write=False)
    return {"N": N, "sel": sel, "msel": msel, "frames": frames}


def shape_case(F: int, n: int, kind: str, m: int) -> dict:
    """One shape: a sigma = 10 A synthetic topology of N atoms, F frames of it with 1 A of noise, tumbled and shifted (related frames: the gap is wide)."""
    return _shape_case(F, n, kind, m)


# ---- reference -----------------------------------------------------------------------------------------------------------------------------------------------
def centre(X: np.ndarray, XM: np.ndarray | None = None) -> tuple:
    """(centred fit atoms [F, n, 3], centroids [F, 3], centred measured atoms or None), on the centroid of the fit atoms, in two steps."""
    X = np.asarray(X, np.float64)
    c0 = X.mean(1, keepdims=True)
    r = (X - c0).mean(1, keepdims=True)
    return (X - c0) - r, (c0 + r)[:, 0], None if XM is None else (np.asarray(XM, np.float64) - c0) - r


def kabsch(Xc: np.ndarray, T: np.ndarray) -> tuple:
    """(R [F, 3, 3] with R x_f ~ T, gap [F] = lambda_1 - lambda_2 of K(S_f)) by the SVD with the determinant sign: S = U s V^T, R = V diag(1, 1, d) U^T."""
    S = np.einsum("fia,ib->fab", Xc, T)
    U, s, Vt = np.linalg.svd(S)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    d[d == 0] = 1.0
    D = np.zeros_like(S)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    return np.einsum("fji,fjk,flk->fil", Vt, D, U), 2.0 * (s[:, 1] + d * s[:, 2])


def rotate(R: np.ndarray, X: np.ndarray) -> np.ndarray:
    return np.einsum("fab,fib->fia", R, X)


def reference(X, XM=None, ref=0, max_rounds: int = 1, tol: float = 0.0) -> dict:
    """Every output of the call in f64 from X [F, n, 3] (the fit atoms), XM [F, m, 3] (the measured atoms; None: X) and ref (a frame index or the reference's
    fit atoms [n, 3]); `changes`: the change of every round; `bound`: the tolerances of the docstring for ONE round at the last round's target; `scale`:
    rounds + 1 for an iterated call, 1 for one round; `gap_ratio`: the smallest gap_f / Gs_f of the last round."""
    X = np.asarray(X, np.float64)
    F, n = X.shape[:2]
    Xc, c, XMc = centre(X, XM)
    if XMc is None:
        XMc = Xc
    if isinstance(ref, (int, np.integer)):
        T, c_t, ref_abs = Xc[ref], c[ref], X[ref]
    else:
        ref_abs = np.asarray(ref, np.float64)
        Tc, ct, _ = centre(ref_abs[None])
        T, c_t = Tc[0], ct[0]
    changes = []
    while True:
        R, gap = kabsch(Xc, T)
        Y = rotate(R, Xc)
        M = Y.mean(0)
        changes.append(float(np.sqrt(((M - T) ** 2).sum() / n)))
        if len(changes) == max_rounds or changes[-1] <= tol:
            break
        T = M
    YM = rotate(R, XMc)
    mean_m = YM.mean(0)
    rmsf = np.sqrt(((YM - mean_m) ** 2).sum(2).mean(0))
    frame = np.sqrt(((Y - M) ** 2).sum(2).mean(1))
    t = c_t - np.einsum("fab,fb->fa", R, c)
    # the bounds
    Gs = (Xc * Xc).sum((1, 2)) + (T * T).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(gap > 0, 2.0 * 64.0 * EPS * Gs / gap, np.inf)
        ratio = np.where(Gs > 0, gap / Gs, 0.0)
    turn = 2.0 * u + 8.0 * EPS
    times = lambda norm: np.where(norm > 0, turn[:, None] * np.where(norm > 0, norm, 1.0), 0.0)   # (an atom on the centroid does not move: 0, also at gap 0)
    tau_fit, tau_m = times(np.linalg.norm(Xc, axis=2)), times(np.linalg.norm(XMc, axis=2))
    big = 4.0 * EPS * max(np.abs(X).max(), np.abs(ref_abs).max(), 0.0 if XM is None else np.abs(XM).max())
    bound = {"aligned": tau_m + big, "mean": tau_m.mean(0) + F * EPS * np.linalg.norm(YM, axis=2).max(0) + big, "rmsf": 2.0 * tau_m.max(0) + 2.0 ** -23 * rmsf,
             "frame_rmsd": 2.0 * tau_fit.max(1) + 2.0 ** -23 * frame, "R": turn, "t": turn * np.linalg.norm(c, axis=1) + big}
    return {"mean": mean_m + c_t, "rmsf": rmsf, "frame_rmsd": frame, "aligned": YM + c_t, "R": R, "t": t, "M": M, "c_t": c_t, "n_rounds": len(changes), "changes": changes,
            "last_change": changes[-1], "bound": bound, "scale": 1.0 if max_rounds == 1 else len(changes) + 1.0, "gap_ratio": float(ratio.min()), "big": big}


def errors(got: dict, ref: dict) -> dict:
    """key -> (error, bound) arrays of every output `got` holds: vector norms for coordinates, the largest entry for R."""
    out = {}
    for key in ("mean", "aligned"):
        if key in got:
            out[key] = (np.linalg.norm(np.asarray(got[key], np.float64) - ref[key], axis=-1), ref["bound"][key] * ref["scale"])
    for key in ("rmsf", "frame_rmsd"):
        out[key] = (np.abs(np.asarray(got[key], np.float64) - ref[key]), ref["bound"][key] * ref["scale"])
    if "transforms" in got:
        tr = np.asarray(got["transforms"], np.float64)
        out["R"] = (np.abs(tr[:, :9].reshape(-1, 3, 3) - ref["R"]).max((1, 2)), ref["bound"]["R"] * ref["scale"])
        out["t"] = (np.linalg.norm(tr[:, 9:] - ref["t"], axis=1), ref["bound"]["t"] * ref["scale"])
    return out


def assert_within(got: dict, ref: dict, what="") -> float:
    """Every output of `got` within the bound of the reference; returns the largest error / bound ratio (0 where both are 0)."""
    worst = 0.0
    for key, (err, bound) in errors(got, ref).items():
        bad = np.argwhere(~(err <= bound))
        if len(bad):
            k = tuple(bad[0])
            raise AssertionError(f"{what} {key}: {len(bad)} entries outside the bound, first {list(k)}: error {err[k]:.3e}, bound {bound[k]:.3e}")
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, 0.0)
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    return worst


def check_rotations(transforms: np.ndarray, what=""):
    """R orthonormal to 16 eps, det = +1."""
    R = np.asarray(transforms, np.float64)[:, :9].reshape(-1, 3, 3)
    off = np.abs(np.einsum("fab,fcb->fac", R, R) - np.eye(3)).max() if len(R) else 0.0
    assert off <= 16.0 * EPS, (what, off)
    assert (np.abs(np.linalg.det(R) - 1.0) <= 16.0 * EPS).all(), (what, np.linalg.det(R))


def assert_rigid(got: dict, ref: dict, shape: np.ndarray, what=""):
    """Frames that are rigid copies of one shape: nothing moves, and the mean is a rigid copy of the shape.  The copies are rigid only to the rounding of their
    own absolute coordinates (a frame 1.6 10^5 A out has coordinates 2^-36 A apart), so the term of absolute coordinates joins the bounds of rmsf and
    frame_rmsd here."""
    assert (got["rmsf"] <= ref["bound"]["rmsf"] + ref["big"]).all(), (what, "rmsf", float(np.max(got["rmsf"])))
    assert (got["frame_rmsd"] <= ref["bound"]["frame_rmsd"] + ref["big"]).all(), (what, "frame_rmsd", float(np.max(got["frame_rmsd"])))
    mean = np.asarray(got["mean"], np.float64)
    fit = reference(np.stack([mean, shape]), ref=0)    # the shape superposed on the mean, in numpy
    apart = np.linalg.norm(fit["aligned"][1] - mean, axis=1)
    assert (apart <= ref["bound"]["mean"] + fit["bound"]["aligned"][1] + ref["big"]).all(), (what, "mean", float(apart.max()))


def plain_rmsd(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """sqrt(mean_i |a_i - b_i|^2) per frame of A [F, n, 3] against B [n, 3] or [F, n, 3]: no fit."""
    return np.sqrt(((np.asarray(A, np.float64) - B) ** 2).sum(-1).mean(-1))


# ---- the degenerate geometries: rmsd_cases.degenerate_cases, one round on frame 0 --------------------------------------------------------------------------------
INVARIANTS_ONLY = ("collinear", "n1", "n2")            # gap 0: any top eigenvector is a right answer, compared on invariants
THROUGH_R = ("drift", "duplicates", "mirror", "n3", "planar", "tumble")


def check_degenerate_reach() -> dict:
    d = rc.degenerate_cases()
    assert sorted(INVARIANTS_ONLY + THROUGH_R) == sorted(d)
    ratios = {name: reference(X)["gap_ratio"] for name, X in d.items()}
    for name in THROUGH_R:
        assert ratios[name] >= MIN_GAP, (name, ratios[name])
    for name in INVARIANTS_ONLY:
        assert ratios[name] <= 1e-9, (name, ratios[name])
    assert np.abs(d["drift"]).max() > 0.5 * ts.DRIFT_REACH
    return ratios


# ---- the iterated mean ---------------------------------------------------------------------------------------------------------------------------------------
def ubq_ensemble(F: int, sigma: float, seed: int) -> np.ndarray:
    """[F, 76, 3]: 1ubq CA with N(0, sigma) of noise per atom and frame, tumbled and shifted."""
    return ensemble(rc.ubq_ca(), F, seed, sigma)


ITERATED = {"ubq_0.3": (lambda: ubq_ensemble(21, 0.3, 41), 1), "ubq_5": (lambda: ubq_ensemble(21, 5.0, 42), None), "clusters": (lambda: rc.cluster_fixture()[0], 2)}
ITERATED_ROUNDS = 50


@lru_cache(maxsize=None)
def iterated_fixture(name: str) -> dict:
    """frames [F, n, 3], numpy's own sequence of changes, `tol` = the geometric mean of changes[k] and changes[k + 1] and `rounds` = k + 2, the rounds a call
    with that tol takes.  k is fixed per fixture; None: the first k whose geometric mean lies below 10^-4 A (the default tol of the Python layer)."""
    make, k = ITERATED[name]
    X = make()
    changes = reference(X, max_rounds=12, tol=0.0)["changes"]
    if k is None:
        k = next(j for j in range(len(changes) - 1) if np.sqrt(changes[j] * changes[j + 1]) < 1e-4)
    X.setflags(write=False)
    return {"frames": X, "changes": changes, "k": k, "tol": float(np.sqrt(changes[k] * changes[k + 1])), "rounds": k + 2}


def check_iterated_reach() -> dict:
    """The sequence is strictly decreasing down to tol and ten times apart around it: no rounding of a change can move n_rounds."""
    out = {}
    for name in ITERATED:
        fx = iterated_fixture(name)
        ch, k = fx["changes"], fx["k"]
        assert all(a > b for a, b in zip(ch[: k + 1], ch[1 : k + 2])), (name, ch)
        assert ch[k] >= 10.0 * ch[k + 1], (name, ch)
        ref = reference(fx["frames"], max_rounds=ITERATED_ROUNDS, tol=fx["tol"])
        assert ref["n_rounds"] == fx["rounds"] and ref["last_change"] <= fx["tol"] < ch[k], (name, ref["n_rounds"], fx["rounds"])
        assert ref["gap_ratio"] >= MIN_GAP, (name, ref["gap_ratio"])
        out[name] = {"changes": ch[: k + 2], "tol": fx["tol"], "rounds": fx["rounds"], "gap_ratio": ref["gap_ratio"]}
    return out


def cap_case() -> np.ndarray:
    """Unrelated synthetic frames: no mean structure to converge to within 50 rounds -- the max_rounds cap ends the call."""
    return rc.synthetic(9, 20, seed=77)


CAP_TOL = 1e-4


def check_cap_reach() -> float:
    ref = reference(cap_case(), max_rounds=ITERATED_ROUNDS, tol=CAP_TOL)
    assert ref["n_rounds"] == ITERATED_ROUNDS and ref["last_change"] > 10.0 * CAP_TOL, (ref["n_rounds"], ref["last_change"])
    return ref["last_change"]


# ---- residues ------------------------------------------------------------------------------------------------------------------------------------------------
def residue_rmsf(keys: list, rmsf: np.ndarray) -> tuple:
    """(sorted distinct keys, sqrt of the unweighted mean of rmsf^2 over each key's atoms, f64)."""
    rows = sorted(set(keys))
    r = np.asarray(rmsf, np.float64)
    return rows, np.array([np.sqrt(np.mean([r[k] ** 2 for k, key in enumerate(keys) if key == row])) for row in rows])


def ubq_residue_keys(idx: np.ndarray) -> list:
    """(chain, resi, insertion) of the atoms idx of tests/data/1ubq.pdb, parsed here."""
    lines = [l for l in (rc.DATA / "1ubq.pdb").read_text().splitlines() if l.startswith(("ATOM  ", "HETATM"))]
    return [(lines[k][21], int(lines[k][22:26]), lines[k][26].strip()) for k in idx]
