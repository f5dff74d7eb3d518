"""Cases and references for the RMSD between the frames of an ensemble (arp_rmsd_matrix, arp_rmsd_reference, arp_rmsd_clusters: rmsd.inl + the host half in
rmsd.cpp).  No product imports: tests/test_rmsd_host.py checks arp_rmsd_host, the input checks and every case's reach on the CPU, tests/test_rmsd_gpu.py
runs the cases on the device.

Reference: numpy f64.  Centre every frame on the centroid of the selected atoms, S = A.T @ B per pair, SVD with the determinant sign:
lambda = s0 + s1 + sign(det U det Vt) s2 (the optimum over proper rotations: a mirror image does not superpose), msd = max(0, (G_f + G_g - 2 lambda) / n).
The gromos loop is cluster_cases.gromos on `matrix <= float32(cutoff)`.

Tolerance (derived, not tuned).  A length-n dot product summed in any order errs by at most n eps sum |a||b|; every entry of K is a sum of at most three
entries of S; lambda moves by at most |dK|.  So for device and reference alike |msd - exact| <= c eps (G_f + G_g) with c a small integer.  With
t = 64 2^-52 (G_f + G_g):  |rmsd_dev - rmsd_ref| <= min(sqrt(t), t / rmsd_ref) + 2^-23 rmsd_ref  (the last term: the one rounding to f32).  For n = 1, G = 0
and the result is exactly 0.  Centring on the f64 centroid makes the bound independent of where the frame sits.

The kernels' constants (rmsd.inl), which the shapes below straddle:
  WAVE  = 16   frame pairs per wave edge (the 16 x 16 of the f64 MFMA)
  TILE  = 32   frames per workgroup tile edge (2 x 2 waves): one workgroup per tile of the upper triangle, the mirror tile written by the same workgroup
  WORD  = 32   neighbour bits per word: a tile row is one word of an adjacency row of ceil(F / 32) words
  STEP  = 4    atoms per MFMA (its K); n_pad is n rounded up to it
  CHUNK = 16   atoms staged through LDS per step of the tile loop
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

import trajectory_shapes as ts
from cluster_cases import NAN_BITS, NONE, gromos  # noqa: F401

WAVE, TILE, WORD, STEP, CHUNK = 16, 32, 32, 4, 16
EPS = 2.0 ** -52
SIGMA = 10.0  # A: the synthetic coordinates
DATA = Path(__file__).resolve().parent / "data"

FRAMES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
ATOMS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257]
CHEAP_FRAMES = [1, 2, 17, 33]   # the F of the cross product F x n; the other F run at n = 5 and n = 65, the other n at F = 33 and F = 65


def check_shape_reach():
    assert {-(-F // WORD) for F in FRAMES} >= {1, 2, 3, 5}                                     # words per adjacency row
    assert {-(-F // TILE) for F in FRAMES} >= {1, 2, 3, 5} and any(F % TILE == 0 for F in FRAMES if F > TILE)
    for edge in (WAVE, TILE, 2 * TILE):
        assert {edge - 1, edge, edge + 1} <= set(FRAMES), edge                                 # wave-tile and workgroup-tile edges from both sides
    assert any(F % TILE and F % TILE < WAVE for F in FRAMES if F > TILE)                        # a last tile whose second wave row is empty
    assert max(FRAMES) > 4 * TILE and max(FRAMES) % TILE                                       # more than one tile off the diagonal, a partial last tile
    for edge in (STEP, CHUNK, 4 * CHUNK):
        assert {edge - 1, edge, edge + 1} <= set(ATOMS), edge                                  # the MFMA step, the LDS chunk and whole chunks from both sides
    assert {1, 2, 3} <= set(ATOMS)                                                             # rank-deficient S: the top eigenvalue of K is double
    assert any(n % CHUNK and n > 2 * CHUNK for n in ATOMS) and max(ATOMS) > 256                # a partial last chunk; more atoms than the pack kernel has lanes
    assert set(CHEAP_FRAMES) <= set(FRAMES)


# ---- reference -------------------------------------------------------------------------------------------------------------------------------------------
def centred(X: np.ndarray) -> tuple:
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(1, keepdims=True)
    return Xc, (Xc * Xc).sum((1, 2))


def top_eigenvalue(S: np.ndarray) -> np.ndarray:
    """lambda of K(S) for S [..., 3, 3] by the SVD with the determinant sign."""
    U, s, Vt = np.linalg.svd(S)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    return s[..., 0] + s[..., 1] + d * s[..., 2]


def reference(X: np.ndarray, Y: np.ndarray | None = None) -> dict:
    """rmsd [F, F'] f64 between the frames of X [F, n, 3] and of Y (default X, the diagonal then exactly 0), G_f + G_g [F, F'] and the tolerance [F, F']."""
    A, GA = centred(X)
    B, GB = (A, GA) if Y is None else centred(Y)
    n = A.shape[1]
    S = np.einsum("fia,gib->fgab", A, B)
    gsum = GA[:, None] + GB[None, :]
    r = np.sqrt(np.maximum(0.0, (gsum - 2.0 * top_eigenvalue(S)) / n))
    if Y is None:
        np.fill_diagonal(r, 0.0)
    return {"rmsd": r, "gsum": gsum, "tol": tolerance(r, gsum)}


def tolerance(r: np.ndarray, gsum: np.ndarray) -> np.ndarray:
    t = 64.0 * EPS * gsum
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(np.sqrt(t), np.where(r > 0, t / r, np.inf)) + 2.0 ** -23 * r


def horn_eigvalsh(X: np.ndarray) -> np.ndarray:
    """The same rmsd by an independent f64 route: eigvalsh of Horn's K(S), entry by entry."""
    A, G = centred(X)
    n = A.shape[1]
    S = np.einsum("fia,gib->fgab", A, A)
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[..., a, b] for a in range(3) for b in range(3))
    K = np.empty(S.shape[:2] + (4, 4))
    K[..., 0, 0], K[..., 1, 1], K[..., 2, 2], K[..., 3, 3] = xx + yy + zz, xx - yy - zz, -xx + yy - zz, -xx - yy + zz
    K[..., 0, 1] = K[..., 1, 0] = yz - zy
    K[..., 0, 2] = K[..., 2, 0] = zx - xz
    K[..., 0, 3] = K[..., 3, 0] = xy - yx
    K[..., 1, 2] = K[..., 2, 1] = xy + yx
    K[..., 1, 3] = K[..., 3, 1] = zx + xz
    K[..., 2, 3] = K[..., 3, 2] = yz + zy
    lam = np.linalg.eigvalsh(K)[..., -1]
    r = np.sqrt(np.maximum(0.0, (G[:, None] + G[None, :] - 2.0 * lam) / n))
    np.fill_diagonal(r, 0.0)
    return r


def assert_within(got, ref: dict, what="") -> float:
    """Every entry of `got` within the tolerance of the reference; returns the largest error / bound ratio (0 where both are 0)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref["rmsd"])
    bad = np.argwhere(~(err <= ref["tol"]))
    if len(bad):
        k = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} entries outside the bound, first {list(k)}: got {got[k]!r}, want {ref['rmsd'][k]!r}, error {err[k]:.3e}, bound {ref['tol'][k]:.3e}")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(ref["tol"] > 0, err / ref["tol"], 0.0)
    return float(ratio.max()) if ratio.size else 0.0


def clusters(matrix: np.ndarray, cutoff, max_clusters: int | None = None) -> dict:
    """Every output of the cluster call from an f32 matrix: the loop of cluster_cases.gromos on matrix <= float32(cutoff)."""
    matrix = np.asarray(matrix, np.float32)
    adj = matrix <= np.float32(cutoff)
    F = len(adj)
    cluster, centre, size = gromos(adj, max_clusters)
    to_centre = np.full(F, NAN_BITS, "<u4").view("<f4")
    got = cluster != NONE
    to_centre[got] = matrix[np.arange(F)[got], centre[cluster[got]]]
    return {"cluster": cluster, "rmsd_to_centre": to_centre, "n_neighbours": adj.sum(1).astype("<u4"), "centre": centre, "cluster_size": size, "n_clusters": len(centre)}


def assert_clusters(got: dict, want: dict, what=""):
    assert got["n_clusters"] == want["n_clusters"], (what, "n_clusters", got["n_clusters"], want["n_clusters"])
    for key in ("cluster", "rmsd_to_centre", "n_neighbours", "centre", "cluster_size"):
        g, w = np.asarray(got[key]), want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
            raise AssertionError(f"{what} {key}: {len(bad)} elements differ, first {bad[0].tolist()}: got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


def cutoffs(matrix: np.ndarray) -> list:
    """0 and the median, the ninth decile and the maximum of the matrix's own off-diagonal values."""
    F = len(matrix)
    if F < 2:
        return [0.0]
    off = np.sort(np.asarray(matrix, np.float32)[~np.eye(F, dtype=bool)])
    return [0.0, float(off[len(off) // 2]), float(off[(len(off) * 9) // 10]), float(off[-1])]


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------
def synthetic(F: int, n: int, seed: int | None = None) -> np.ndarray:
    """[F, n, 3] seeded normal coordinates, sigma = 10 A."""
    return np.random.default_rng(1000003 * F + n if seed is None else seed).normal(scale=SIGMA, size=(F, n, 3))


def ubq_atoms() -> list:
    """(atom name, residue name, element, chain, [x, y, z]) of every ATOM / HETATM record of tests/data/1ubq.pdb, parsed here."""
    out = []
    for line in (DATA / "1ubq.pdb").read_text().splitlines():
        if line.startswith(("ATOM  ", "HETATM")):
            out.append((line[12:16].strip(), line[17:20].strip(), line[76:78].strip(), line[21], [float(line[30:38]), float(line[38:46]), float(line[46:54])]))
    return out


def ubq_selection(atoms: str) -> np.ndarray:
    rec = ubq_atoms()
    keep = {"ca": lambda a: a[0] == "CA", "backbone": lambda a: a[0] in ("N", "CA", "C", "O"), "heavy": lambda a: a[2] not in ("H", "D"), "all": lambda a: True}[atoms]
    return np.array([k for k, a in enumerate(rec) if a[1] != "HOH" and keep(a)], "<u4")


def ubq_xyz() -> np.ndarray:
    return np.array([a[4] for a in ubq_atoms()], np.float64)


def ubq_ca() -> np.ndarray:
    return ubq_xyz()[ubq_selection("ca")]


def mirror(frame: np.ndarray) -> np.ndarray:
    return np.asarray(frame, np.float64) * np.array([1.0, 1.0, -1.0])


def degenerate_cases() -> dict:
    """name -> [F, n, 3].  Everything with a double (or worse) top eigenvalue of K: what a Newton iteration on the quartic loses sqrt(eps) on."""
    rng = np.random.default_rng(20)
    ca = ubq_ca()
    one = synthetic(1, 40, seed=21)[0]
    out = {"duplicates": np.stack([one, one, one + 0.0, synthetic(1, 40, seed=22)[0], one])}
    out["mirror"] = np.stack([ca, mirror(ca), ca @ ts.random_rotation(rng).T, mirror(ca) @ ts.random_rotation(rng).T + 7.0])
    flat = synthetic(6, 30, seed=23)
    flat[..., 2] = 0.0
    out["planar"] = np.stack([f @ ts.random_rotation(rng).T for f in flat[:3]] + list(flat[3:]))
    rod = np.zeros((5, 20, 3))
    rod[..., 0] = np.arange(20) * 3.8 + rng.normal(scale=0.2, size=(5, 20))
    out["collinear"] = np.stack([r @ ts.random_rotation(rng).T + rng.normal(scale=30.0, size=3) for r in rod[:3]] + list(rod[3:]))
    for n in (1, 2, 3):
        out[f"n{n}"] = synthetic(7, n, seed=30 + n)
    out["tumble"] = ts.tumble(ca, 9)
    out["drift"] = ts.drift(ca, 9)
    return out


def check_degenerate_reach():
    d = degenerate_cases()
    m = reference(d["mirror"])["rmsd"]
    assert m[0, 1] > 1.0 and m[0, 2] < 1e-6 and m[1, 3] < 1e-6 and abs(m[0, 3] - m[0, 1]) < 1e-6   # a mirror image does not superpose; a rotated copy does
    assert reference(d["duplicates"])["rmsd"][0, 1] == 0.0 or reference(d["duplicates"])["rmsd"][0, 1] < 1e-6
    for name in ("planar", "collinear", "n1", "n2", "n3"):   # the two largest eigenvalues of K coincide: s2 = 0
        A, _ = centred(d[name])
        s = np.linalg.svd(np.einsum("ia,ib->ab", A[0], A[1]), compute_uv=False)
        assert s[2] <= 1e-9 * max(s[0], 1e-300), (name, s)
    for name in ("tumble", "drift"):
        r = reference(d[name])
        assert r["rmsd"].max() < 1e-4 and (r["rmsd"] <= r["tol"]).all(), name
    assert np.abs(d["drift"]).max() > 0.5 * ts.DRIFT_REACH


# ---- the cluster fixture: five well separated states of 1ubq CA ----------------------------------------------------------------------------------------------
CLUSTER_CUTOFF = 1.0
CLUSTER_SIZES = [17, 16, 15, 14, 13]


def cluster_fixture() -> tuple:
    """(frames [75, 76, 3], state [75]).  State k = 1ubq CA + N(0, 1.5 A), 13 + k members; each member adds N(0, 0.15 A) noise, a random rotation and a random
    translation; the frames are shuffled."""
    rng = np.random.default_rng(5)
    ca = ubq_ca()
    frames, state = [], []
    for k in range(5):
        centre = ca + rng.normal(scale=1.5, size=ca.shape)
        for _ in range(13 + k):
            frames.append((centre + rng.normal(scale=0.15, size=ca.shape)) @ ts.random_rotation(rng).T + rng.normal(scale=50.0, size=3))
            state.append(k)
    order = rng.permutation(len(frames))
    return np.array(frames)[order], np.array(state)[order]


def check_cluster_fixture() -> dict:
    """The fixture's separation on the reference: members of a state lie well inside the cutoff, different states well outside, and no pair within the
    tolerance of the cutoff -- the neighbour relation of any correct implementation is the reference's, with zero excluded pairs."""
    frames, state = cluster_fixture()
    ref = reference(frames)
    same = state[:, None] == state[None, :]
    off = ~np.eye(len(state), dtype=bool)
    within, between = ref["rmsd"][same & off].max(), ref["rmsd"][~same].min()
    # noise of 0.15 A per coordinate on both members: about 0.15 sqrt(6) = 0.37 A; states 1.5 A apart per coordinate: about 1.5 sqrt(6) = 3.7 A
    assert within <= 0.45 and between >= 3.2, (within, between)
    assert (np.abs(ref["rmsd"] - CLUSTER_CUTOFF) > ref["tol"] + 2.0 ** -23).all()
    want = clusters(ref["rmsd"].astype(np.float32), CLUSTER_CUTOFF)
    assert want["n_clusters"] == 5 and want["cluster_size"].tolist() == CLUSTER_SIZES
    assert all(len(set(state[want["cluster"] == k])) == 1 for k in range(5))
    return {"within": float(within), "between": float(between), "want": want}
