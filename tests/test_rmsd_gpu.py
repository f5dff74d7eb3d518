"""RMSD between the frames of an ensemble (arp_rmsd_matrix, arp_rmsd_reference, arp_rmsd_clusters) on the device.

k_rmsd_pack / k_rmsd_gram / k_rmsd_to_centre at every wave-tile, workgroup-tile, MFMA-step and LDS-chunk edge of tests/rmsd_cases.py: the matrix within the
derived bound of numpy and of arp_rmsd_host, exactly symmetric, identical bytes from call to call and from pass size to pass size; the geometries whose top
eigenvalue is double; the reference call against the matrix's rows, bit for bit; the clusters against cluster_cases.gromos on the device's own matrix, byte
for byte, and against the independent reference on a fixture whose neighbour relation no rounding can change.  Expected values never come from the call under
test, except where bit-equality between two calls is the property.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import rmsd_cases as rc
import trajectory_shapes as ts
from arpeggia_amd import _lib

pytestmark = pytest.mark.gpu

KNOBS = ("rmsd_chunk_atoms", "rmsd_cap_bytes")
WORST = {"ratio": 0.0, "what": None}   # the largest error / bound of the device over every case of this module (printed by the last test)
NEAR_ZERO = {"ratio": 0.0, "what": None}   # the same over the off-diagonal pairs whose reference rmsd is below 10^-3 A, where no f32 rounding term hides the f64 error


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


def topology(N: int, models: np.ndarray | None = None) -> aa.Structure:
    """N CA atoms of N glycines in chain A; models [F, N, 3]: a multi-model structure whose models are the frames."""
    F = 1 if models is None else len(models)
    atoms = [("GLY", "CA", "C", "A", k + 1, (3.8 * k, 0.0, 0.0) if models is None else tuple(models[f, k])) for f in range(F) for k in range(N)]
    rec = ts.records(atoms)
    rec["serial"] = np.tile(np.arange(1, N + 1), F).astype(rec["serial"].dtype)
    rec["model_serial"] = np.repeat(np.arange(1, F + 1), N).astype(rec["model_serial"].dtype)
    return aa.Structure.from_records(rec)


def embed(X: np.ndarray) -> tuple:
    """(structure, frames [F, N, 3], sel): the n atoms of X among N = n + 2, with two decoys the selection skips (the pack kernel gathers)."""
    F, n = X.shape[:2]
    N = n + 2
    sel = np.delete(np.arange(N), [0, N // 2]).astype("<u4")
    frames = np.random.default_rng(n).normal(scale=100.0, size=(F, N, 3))
    frames[:, sel] = X
    return topology(N), frames, sel


def note(ratio: float, what):
    if ratio > WORST["ratio"]:
        WORST.update(ratio=ratio, what=what)


def check_matrix(ctx, X: np.ndarray, what, passes: bool = False) -> np.ndarray:
    s, frames, sel = embed(X)
    F, N = frames.shape[:2]
    got = ctx.rmsd_matrix(s, frames, atoms=sel)
    assert got.dtype == np.float32 and got.shape == (F, F)
    ref = rc.reference(X)
    note(rc.assert_within(got, ref, (what, "numpy")), what)
    near = (ref["rmsd"] < 1e-3) & ~np.eye(F, dtype=bool) & (ref["tol"] > 0)   # superposable pairs: the f64 term of the bound, sqrt(t), is all there is
    if near.any() and X.shape[1] > 1:
        ratio = float((np.abs(got - ref["rmsd"])[near] / ref["tol"][near]).max())
        if ratio > NEAR_ZERO["ratio"]:
            NEAR_ZERO.update(ratio=ratio, what=what)
    host =aa.rmsd_host(X).astype(np.float64)
    rc.assert_within(got, {"rmsd": host, "tol": rc.tolerance(host, ref["gsum"])}, (what, "host"))
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes(), (what, "symmetric")
    assert (np.diag(got).view("<u4") == 0).all(), (what, "diagonal")
    assert got.tobytes() == ctx.rmsd_matrix(s, frames, atoms=sel).tobytes(), (what, "two calls")
    if passes:
        for per in sorted({F, -(-F // 2), 1}):   # 1, 2 and F passes
            aa.debug_set("rmsd_chunk_atoms", per * N)
            assert got.tobytes() == ctx.rmsd_matrix(s, frames, atoms=sel).tobytes(), (what, "frames per pass", per)
        aa.debug_set("rmsd_chunk_atoms", 0)
    if X.shape[1] == 1:
        assert (got == 0).all(), what
    return got


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", rc.FRAMES)
def test_matrix_shapes(ctx, F):
    """The cross product F x n where F is cheap, n = 5 and 65 elsewhere; forced passes at n = 5."""
    for n in (rc.ATOMS if F in rc.CHEAP_FRAMES else (5, 65)):
        check_matrix(ctx, rc.synthetic(F, n), (F, n), passes=n == 5)


@pytest.mark.parametrize("n", rc.ATOMS)
def test_matrix_atoms(ctx, n):
    """Every n at two and three tiles; forced passes at F = 65."""
    for F in (33, 65):
        check_matrix(ctx, rc.synthetic(F, n), (F, n), passes=F == 65)


@pytest.mark.parametrize("name", sorted(rc.degenerate_cases()))
def test_degenerate_geometry(ctx, name):
    """A double top eigenvalue of K: within the same bound (what a Newton iteration on the quartic fails)."""
    X = rc.degenerate_cases()[name]
    got = check_matrix(ctx, X, name, passes=True)
    if name == "mirror":
        assert got[0, 1] > 1.0 and got[0, 2] < 1e-5 and abs(float(got[0, 3]) - float(got[0, 1])) < 1e-5
    if name in ("tumble", "drift"):
        assert got.max() < 1e-4


# ---- the reference call ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,n", [(1, 3), (17, 5), (65, 17), (130, 65)])
def test_reference_rows(ctx, F, n):
    X = rc.synthetic(F, n)
    s, frames, sel = embed(X)
    matrix = ctx.rmsd_matrix(s, frames, atoms=sel)
    ref = rc.reference(X)
    for k in sorted({0, F - 1, min(F - 1, rc.TILE + 3), F // 2}):   # first, last, one in another tile
        row = ctx.rmsd(s, frames, reference=k, atoms=sel)
        assert row.dtype == np.float32 and row.tobytes() == matrix[k].tobytes(), (F, n, k)
        ext = ctx.rmsd(s, frames, reference=frames[k], atoms=sel)   # the same coordinates as an [N, 3] array: every entry is computed
        keep = np.arange(F) != k
        assert ext[keep].tobytes() == matrix[k][keep].tobytes(), (F, n, k)
        assert abs(float(ext[k])) <= np.sqrt(64.0 * rc.EPS * ref["gsum"][k, k]), (F, n, k, ext[k])
    other = rc.synthetic(1, n, seed=F + 77)
    ref_frame = np.random.default_rng(3).normal(scale=50.0, size=frames.shape[1:])
    ref_frame[sel] = other[0]
    got = ctx.rmsd(s, frames, reference=ref_frame, atoms=sel)
    note(rc.assert_within(got[None, :], rc.reference(other, X), (F, n, "a reference that is no frame")), (F, n, "reference"))


# ---- clusters, exact: every output from the device's own matrix ----------------------------------------------------------------------------------------------
def check_clusters(ctx, X: np.ndarray, what, cutoffs=None, caps=(None,)):
    s, frames, sel = embed(X)
    matrix = ctx.rmsd_matrix(s, frames, atoms=sel)
    for cutoff in (rc.cutoffs(matrix) if cutoffs is None else cutoffs):
        for cap in caps:
            got = ctx.rmsd_clusters(s, frames, atoms=sel, cutoff=cutoff, max_clusters=cap)
            want = rc.clusters(matrix, cutoff, cap)
            rc.assert_clusters(got, want, (what, cutoff, cap))
            assert (got["n_neighbours"] == (matrix <= np.float32(cutoff)).sum(1)).all()
            left = got["cluster"] == rc.NONE
            assert (got["rmsd_to_centre"].view("<u4")[left] == rc.NAN_BITS).all() and (got["rmsd_to_centre"][got["centre"]].view("<u4") == 0).all()
    return matrix


@pytest.mark.parametrize("F", rc.FRAMES)
def test_clusters_shapes(ctx, F):
    for n in (3, 17):
        check_clusters(ctx, rc.synthetic(F, n), (F, n))


def test_clusters_of_groups(ctx):
    """Tight groups far apart (more than one non-trivial cluster, frames in three tiles), and max_clusters = 1, 2, C, C + 1."""
    rng = np.random.default_rng(9)
    base = rc.synthetic(4, 20, seed=90)
    X = np.stack([base[k % 4] + rng.normal(scale=0.05 * (1 + k % 3), size=(20, 3)) for k in range(70)])
    matrix = check_clusters(ctx, X, "groups")
    cutoff = 1.0   # noise of at most 0.15 A per coordinate inside a group, unrelated sigma = 10 A shapes between groups
    C = rc.clusters(matrix, cutoff)["n_clusters"]
    assert C == 4
    check_clusters(ctx, X, "groups, capped", cutoffs=[cutoff], caps=(1, 2, C, C + 1))
    s, frames, sel = embed(X)
    capped = ctx.rmsd_clusters(s, frames, atoms=sel, cutoff=cutoff, max_clusters=1)
    assert capped["n_clusters"] == 1 and (capped["cluster"] == rc.NONE).any()


def test_cutoff_is_inclusive_and_compared_as_f32(ctx):
    X = rc.synthetic(40, 9)
    s, frames, sel = embed(X)
    matrix = ctx.rmsd_matrix(s, frames, atoms=sel)
    v = np.float32(matrix[3, 37])   # an attained value, in the mirror tile
    below = np.nextafter(v, np.float32(0.0), dtype=np.float32)
    at = ctx.rmsd_clusters(s, frames, atoms=sel, cutoff=float(v))
    under = ctx.rmsd_clusters(s, frames, atoms=sel, cutoff=float(below))
    count = lambda c: int((matrix[3] <= np.float32(c)).sum())
    assert at["n_neighbours"][3] == count(v) == under["n_neighbours"][3] + 1 and at["n_neighbours"][37] == under["n_neighbours"][37] + 1
    rc.assert_clusters(at, rc.clusters(matrix, v), "at")
    rc.assert_clusters(under, rc.clusters(matrix, below), "under")


# ---- clusters against the independent reference --------------------------------------------------------------------------------------------------------------
def test_cluster_fixture(ctx):
    """Five states of 1ubq CA, 75 frames: no pair lies within the bound of the cutoff, so the clustering is numpy's exactly: 5 clusters of 17, 16, 15, 14, 13."""
    want = rc.check_cluster_fixture()["want"]
    frames, _ = rc.cluster_fixture()
    s = topology(frames.shape[1])
    got = ctx.rmsd_clusters(s, frames, atoms="ca", cutoff=rc.CLUSTER_CUTOFF)
    assert got["n_clusters"] == 5 and got["cluster_size"].tolist() == rc.CLUSTER_SIZES
    for key in ("cluster", "n_neighbours", "centre", "cluster_size"):
        assert np.array_equal(got[key], want[key]), key
    ref = rc.reference(frames)
    to_centre = {"rmsd": ref["rmsd"][np.arange(75), want["centre"][want["cluster"]]][None], "tol": ref["tol"][np.arange(75), want["centre"][want["cluster"]]][None]}
    note(rc.assert_within(got["rmsd_to_centre"][None], to_centre, "fixture"), "fixture")


# ---- capacity ------------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity(ctx):
    X = rc.synthetic(40, 4)
    s, frames, sel = embed(X)
    aa.debug_set("rmsd_cap_bytes", 40 * 40 * 4 - 1)   # the packed frames (40 x 3 x 4 x 8 + 320 bytes) and the neighbour bits (40 x 2 x 4) fit, the matrix does not
    with pytest.raises(aa.ArpeggiaError) as e:
        ctx.rmsd_matrix(s, frames, atoms=sel)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "40 frames (F)" in str(e.value) and "6400 bytes" in str(e.value) and "rmsd_cap_bytes" in str(e.value)
    got = ctx.rmsd_clusters(s, frames, atoms=sel, cutoff=10.0)   # the cluster call still runs at an F whose matrix is refused
    assert len(ctx.rmsd(s, frames, atoms=sel)) == 40
    aa.debug_set("rmsd_cap_bytes", 0)
    rc.assert_clusters(got, rc.clusters(ctx.rmsd_matrix(s, frames, atoms=sel), 10.0), "capacity")
    aa.debug_set("rmsd_cap_bytes", 1000)   # below the packed frames: every call names F, n and the bytes
    for call in (lambda: ctx.rmsd(s, frames, atoms=sel), lambda: ctx.rmsd_clusters(s, frames, atoms=sel, cutoff=1.0)):
        with pytest.raises(aa.ArpeggiaError) as e:
            call()
        assert e.value.status == _lib.ARP_ERR_CAPACITY and "40 frames (F) x 4 selected atoms (n) need 4160 bytes" in str(e.value)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_1ubq(ctx, ubq_path):
    s = aa.Structure.load(ubq_path)
    base = rc.ubq_xyz()
    frames = ts.jitter(base, 21, seed=11)
    for atoms, n in (("ca", 76), ("heavy", 602), (rc.ubq_selection("backbone"), 304)):
        sel = aa.rmsd_select(s, atoms)
        assert len(sel) == n
        matrix = aa.get_rmsd_matrix(s, frames, atoms=atoms)
        note(rc.assert_within(matrix, rc.reference(frames[:, sel]), ("1ubq", n)), ("1ubq", n))
        assert matrix.tobytes() == ctx.rmsd_matrix(s, frames, atoms=sel).tobytes()
        assert aa.get_rmsd(s, frames, atoms=atoms).tobytes() == matrix[0].tobytes() and aa.get_rmsd(s, frames, reference=20, atoms=atoms).tobytes() == matrix[20].tobytes()
        cutoff = float(np.median(matrix))
        rc.assert_clusters(aa.get_rmsd_clusters(s, frames, atoms=atoms, cutoff=cutoff), rc.clusters(matrix, cutoff), ("1ubq", n))
    one = aa.get_rmsd_matrix(s)   # the file's one model is the one frame
    assert one.shape == (1, 1) and one[0, 0] == 0


def test_end_to_end_models_are_the_frames(ctx):
    X = rc.synthetic(9, 12, seed=4)
    s = topology(12, X)
    matrix = aa.get_rmsd_matrix(s, atoms="ca")
    assert matrix.shape == (9, 9)
    note(rc.assert_within(matrix, rc.reference(X), "models"), "models")
    assert matrix.tobytes() == aa.get_rmsd_matrix(topology(12), X, atoms="all").tobytes()
    assert aa.get_rmsd(s, reference=4).tobytes() == matrix[4].tobytes()
    cutoff = float(np.median(matrix))
    rc.assert_clusters(aa.get_rmsd_clusters(s, cutoff=cutoff), rc.clusters(matrix, cutoff), "models")


def test_worst_ratio_is_reported(ctx):
    """Runs last: the largest error / bound ratio of the device over every case above (profiles/ records it)."""
    print(f"largest device error / bound: {WORST['ratio']:.4f} at {WORST['what']}; over superposable pairs: {NEAR_ZERO['ratio']:.4f} at {NEAR_ZERO['what']}")
    assert WORST["ratio"] <= 1.0 and NEAR_ZERO["ratio"] <= 1.0
