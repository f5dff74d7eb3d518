"""Covariance, DCCM and projection (arp_covariance, arp_project) on the device.

k_cov_dev / k_cov_gram<kCovFull, kCovDccm> / k_cov_finish / k_dccm_var / k_dccm_finish / k_project at every pad, wave, tile, chunk and slab edge of
tests/cov_cases.py: cov, dccm and proj within the derived bounds of numpy and of the host yardsticks, on every shape and on the closed-form fixture; the
invariants of the device's own outputs (symmetric bits, the dccm's diagonal and range, block traces against rmsf^2 of the same call, the smallest eigenvalue,
the projections' sum and variance against the eigenvalues); identical bytes from call to call, from pass size to pass size, with and without the other output,
and against arp_rmsf for everything that call returns; the capacity error; 1ubq CA end to end through pca() and the command line.
Expected values never come from the call under test, except where bit-equality between two calls is the property.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import cov_cases as cc
import rmsd_cases as rc
import rmsf_cases as fc
import trajectory_shapes as ts
from arpeggia_amd import _lib

pytestmark = pytest.mark.gpu

KNOBS = ("rmsd_chunk_atoms", "rmsd_cap_bytes")
WORST = {"cov": 0.0, "cov_what": None, "proj": 0.0, "proj_what": None, "iterated": 0.0, "iterated_what": None}
RMSF_KEYS = ("atom", "mean", "rmsf", "frame_rmsd", "transforms", "bfactor")
IDS = lambda s: f"F{s[0]}-n{s[1]}-{s[2]}-m{s[3]}"
EPS = cc.EPS


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


def atom_records(N: int, models: np.ndarray | None = None) -> dict:
    """N CA atoms of N glycines in chain A; models [F, N, 3]: a multi-model structure whose models are the frames."""
    F = 1 if models is None else len(models)
    atoms = [("GLY", "CA", "C", "A", k + 1, (3.8 * k, 0.0, 0.0) if models is None else tuple(models[f, k])) for f in range(F) for k in range(N)]
    rec = ts.records(atoms)
    rec["serial"] = np.tile(np.arange(1, N + 1), F).astype(rec["serial"].dtype)
    rec["model_serial"] = np.repeat(np.arange(1, F + 1), N).astype(rec["model_serial"].dtype)
    return rec


def topology(N: int, models: np.ndarray | None = None) -> aa.Structure:
    return aa.Structure.from_records(atom_records(N, models))


def note(ratio: float, what, key="cov"):
    if ratio > WORST[key]:
        WORST[key], WORST[key + "_what"] = ratio, what


def call(ctx, c: dict, reference=0, cov=True, dccm=True, **kw) -> dict:
    return ctx.covariance(topology(c["N"]), c["frames"], fit=c["sel"], atoms=c["msel"], reference=reference, cov=cov, dccm=dccm, transforms=True, **kw)


def same_bytes(a: dict, b: dict, what, keys=("covariance", "dccm") + RMSF_KEYS):
    for key in keys:
        if key in a or key in b:
            assert a[key].tobytes() == b[key].tobytes(), (what, key)
    assert a["n_rounds"] == b["n_rounds"] and a["last_change"] == b["last_change"], what


def measured(c: dict) -> tuple:
    """(fit coordinates, measured coordinates or None, the measured atoms' absolute coordinates, their indices)."""
    X = c["frames"][:, c["sel"]]
    idx = c["sel"] if c["msel"] is None else c["msel"]
    return X, None if c["msel"] is None else c["frames"][:, c["msel"]], c["frames"][:, idx], idx


def check_own_outputs(got: dict, F: int, m: int, what, cov_bound=None):
    """What holds of the device's outputs among themselves.  The trace of atom i's block and rmsf_i^2 are two sums of the same 3 F squares d^2 -- k_cov_dev
    forms d by k_rmsf_sweep's expressions, the same bits -- so they differ by the rounding of two sums of 3 F non-negative terms, (3 F + 8) eps v, and by
    rmsf's one rounding to f32 (2^-24 on rmsf, 2^-23 on its square; 2^-22 leaves room for the f64 square root)."""
    cc.check_matrices(got, m, what)
    if "covariance" in got:
        trace = np.diag(got["covariance"]).reshape(m, 3).sum(1)
        r2 = got["rmsf"].astype(np.float64) ** 2
        assert (np.abs(trace - r2) <= ((3 * F + 8) * EPS + 2.0 ** -22) * np.maximum(trace, r2)).all(), (what, "block traces", float(np.abs(trace - r2).max()))
        if cov_bound is not None:
            low = float(np.linalg.eigvalsh(got["covariance"])[0])
            assert low >= -3 * m * float(cov_bound.max()), (what, "smallest eigenvalue", low)


def host_chain(c: dict, ref: dict, reference=0) -> tuple:
    """The yardsticks end to end, arp_rmsf_host then arp_covariance_host, and the sum of both sides' bounds against numpy: the device's, and the yardstick's,
    whose deviations carry the same tau and the rounding of the absolute coordinates they are formed from."""
    X, XM, _, _ = measured(c)
    host = aa.rmsf_host(X, XM, reference=reference)
    hc = aa.covariance_host(host["aligned"], host["mean"], cov=True, dccm=True)
    b = cc.second_moments(ref["D"], ref["tau"] + ref["base"]["big"])
    return hc, {"covariance": b["cov_bound"], "dccm": b["dccm_bound"]}


# ---- every shape ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.shapes(), ids=IDS)
def test_shapes(ctx, case):
    F, n, kind, m = case
    c = fc.shape_case(*case)
    got = call(ctx, c)
    through = n > 2
    ref = cc.reference(case) if through else None
    check_own_outputs(got, F, m, case, None if not through or cc.cov_only(case) else ref["cov_bound"])
    # everything arp_rmsf returns, byte for byte
    rm = ctx.rmsf(topology(c["N"]), c["frames"], fit=c["sel"], atoms=c["msel"], reference=0, transforms=True)
    same_bytes(got, rm, (case, "arp_rmsf"), RMSF_KEYS)
    same_bytes(got, call(ctx, c), (case, "two calls"))
    same_bytes(got, call(ctx, c, cov=False), (case, "dccm without cov"), ("dccm",) + RMSF_KEYS)
    same_bytes(got, call(ctx, c, dccm=False), (case, "cov without dccm"), ("covariance",) + RMSF_KEYS)
    if kind != "same" or n in (5, 33):
        N = c["N"]
        for per in sorted({F, -(-F // 2), 1}):   # 1, 2 and F passes
            aa.debug_set("rmsd_chunk_atoms", per * N)
            same_bytes(got, call(ctx, c), (case, "frames per pass", per))
        aa.debug_set("rmsd_chunk_atoms", 0)
    if cc.cov_only(case):
        assert (got["covariance"] == 0).all() and (got["dccm"] == np.eye(m, dtype=np.float32)).all() and (got["rmsf"] == 0).all()
        return
    if not through:
        return
    note(cc.assert_within(got, ref, (case, "numpy")), case)
    hc, slack = host_chain(c, ref)
    cc.assert_within(got, dict(ref, cov=hc["covariance"], dccm=hc["dccm"].astype(np.float64)), (case, "host"), slack=slack)


def test_other_references(ctx):
    """A reference frame in another slab; a reference that is no frame."""
    case = (65, 64, "overlap", 31)
    c = fc.shape_case(*case)
    X, XM, _, _ = measured(c)
    for k in (5, 64):
        got = call(ctx, c, reference=k)
        note(cc.assert_within(got, cc.reference_of(X, XM, ref=k), ("frame", k)), ("frame", k))
    other = c["frames"][7] + np.random.default_rng(1).normal(scale=0.5, size=c["frames"][7].shape) + 40.0
    got = call(ctx, c, reference=other)
    note(cc.assert_within(got, cc.reference_of(X, XM, ref=other[c["sel"]]), "external"), "external")


def test_closed_form(ctx):
    fx, b = cc.closed_form(), cc.closed_form_bounds()
    got = call(ctx, fx, reference=fx["ref_xyz"])
    check_own_outputs(got, len(fx["frames"]), len(fx["msel"]), "closed form", b["cov_bound"])
    ratio = cc.assert_within(got, dict(cov=fx["cov"], dccm=fx["dccm"], cov_bound=b["cov_bound"], dccm_bound=b["dccm_bound"]), "closed form")
    print(f"closed form: largest device error / bound {ratio:.4f}")
    note(ratio, "closed form")
    assert set(np.unique(np.round(got["dccm"].astype(np.float64), 5))) == {-1.0, 0.0, 1.0}


def test_rigid_shape_does_not_move(ctx):
    X, b = cc.rigid_case(), cc.rigid_bound()
    F, n = X.shape[:2]
    N, sel, _ = fc.layout(n, "same", n)
    frames = np.random.default_rng(n).normal(scale=100.0, size=(F, N, 3))
    frames[:, sel] = X
    got = call(ctx, {"N": N, "sel": sel, "msel": None, "frames": frames})
    cc.check_matrices(got, n, "rigid")
    assert (np.abs(got["covariance"]) <= b["cov_bound"]).all(), float(np.abs(got["covariance"]).max())


def test_iterated_mean(ctx):
    fx = fc.iterated_fixture("ubq_0.3")
    X = np.array(fx["frames"])
    F, n = X.shape[:2]
    N, sel, _ = fc.layout(n, "same", n)
    frames = np.random.default_rng(n).normal(scale=100.0, size=(F, N, 3))
    frames[:, sel] = X
    c = {"N": N, "sel": sel, "msel": None, "frames": frames}
    got = call(ctx, c, reference="mean", max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"])
    ref = cc.reference_of(X, max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"])
    assert got["n_rounds"] == ref["base"]["n_rounds"] == fx["rounds"] and got["converged"]
    assert (ref["v"] >= cc.MIN_SIGNAL * ref["v_bound"]).all()
    note(cc.assert_within(got, ref, "iterated"), "ubq_0.3", "iterated")
    rm = ctx.rmsf(topology(N), frames, fit=sel, reference="mean", max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"], transforms=True)
    same_bytes(got, rm, "iterated, arp_rmsf", RMSF_KEYS)
    check_own_outputs(got, F, n, "iterated", ref["cov_bound"])


# ---- projection ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.shapes(), ids=IDS)
def test_projection(ctx, case):
    """Every shape, numpy's own transforms and mean as the inputs; k at 1, 15, 16, 17 and 3 m; against numpy and against arp_project_host (both sides'
    bounds); two calls, and 1, 2 and F upload passes, give the same bytes."""
    F, n, kind, m = case
    c = fc.shape_case(*case)
    base = cc.reference(case)["base"]
    _, _, P, idx = measured(c)
    s = topology(c["N"])
    tr = np.concatenate([base["R"].reshape(F, 9), base["t"]], axis=1)
    for k in cc.mode_counts(m):
        V = cc.random_modes(m, k)
        want = cc.projection(P, tr, base["mean"], V, base["big"])
        got = ctx.project(s, c["frames"], idx, base["mean"], V, tr)
        assert got.shape == (F, k) and got.dtype == np.float64
        note(cc.ratio_within(got, want["proj"], want["bound"], (case, k, "numpy")), (case, k), "proj")
        cc.ratio_within(got, aa.project_host(P, base["mean"], V, tr), 2.0 * want["bound"], (case, k, "host"))
        assert got.tobytes() == ctx.project(s, c["frames"], idx, base["mean"], V, tr).tobytes(), (case, k, "two calls")
    if kind != "same" or n in (5, 33):
        for per in sorted({F, -(-F // 2), 1}):
            aa.debug_set("rmsd_chunk_atoms", per * c["N"])
            assert got.tobytes() == ctx.project(s, c["frames"], idx, base["mean"], V, tr).tobytes(), (case, "frames per pass", per)


def test_closed_form_projection(ctx):
    """The unit modes return the deviations themselves, which the fixture knows in closed form: no numerical reference.  The transforms and the mean come
    from arp_rmsf on the same frames."""
    fx, want = cc.closed_form(), cc.closed_form_projection()
    s = topology(fx["N"])
    rm = ctx.rmsf(s, fx["frames"], fit=fx["sel"], atoms=fx["msel"], reference=fx["ref_xyz"], aligned=True, transforms=True)
    got = ctx.project(s, fx["frames"], fx["msel"], rm["mean"], want["modes"], rm["transforms"])
    ratio = cc.ratio_within(got, want["proj"], want["bound"], "closed form")
    print(f"closed form: largest projection error / bound {ratio:.4f}")
    note(ratio, "closed form", "proj")
    placed = np.zeros_like(fx["frames"])
    placed[:, fx["msel"]] = rm["aligned"]
    cc.ratio_within(ctx.project(s, placed, fx["msel"], rm["mean"], want["modes"], None), want["proj"], want["bound"], "closed form, superposed frames")


def test_projection_of_superposed_frames(ctx):
    """transforms=None on the aligned coordinates of rmsf against the call with the transforms on the raw frames: the two routes to R p + t differ by the
    rounding of absolute coordinates on either side, twice the bound's term and twice its summation term."""
    case = (65, 64, "overlap", 31)
    c = fc.shape_case(*case)
    _, _, P, idx = measured(c)
    s = topology(c["N"])
    rm = ctx.rmsf(s, c["frames"], fit=c["sel"], atoms=c["msel"], reference=0, aligned=True, transforms=True)
    V = cc.random_modes(31, 17)
    raw = ctx.project(s, c["frames"], idx, rm["mean"], V, rm["transforms"])
    placed = np.zeros_like(c["frames"])
    placed[:, idx] = rm["aligned"]
    done = ctx.project(s, placed, idx, rm["mean"], V, None)
    big = 4.0 * EPS * max(np.abs(c["frames"]).max(), np.abs(rm["aligned"]).max(), np.abs(rm["transforms"][:, 9:]).max())
    want = cc.projection(P, rm["transforms"], rm["mean"], V, big)
    note(cc.ratio_within(raw, want["proj"], want["bound"], "device transforms"), "device transforms", "proj")
    cc.ratio_within(done, raw, 2.0 * want["bound"], "superposed frames")
    again = cc.projection(rm["aligned"], None, rm["mean"], V, big)
    cc.ratio_within(done, again["proj"], again["bound"], "identity")


@pytest.mark.parametrize("case", [(65, 33, "same", 33), (33, 20, "disjoint", 65), (200, 16, "overlap", 17)], ids=IDS)
def test_pca_invariants(ctx, case):
    """pca() on the device's own outputs.  D' = R p + t - mean under the device's transforms and mean, exactly; the device's deviations are D' to the
    rounding of absolute coordinates on either route (2 big), so |cov - D'^T D' / F| <= B = the cov bound at tau = 2 big, and proj is D' V^T to its bound pb.
      sum_f proj_fj = 0:  sum_f D'_fa = F (mean'_a - mean_a), where mean' is the exact mean of R p + t: the device's mean is a sum of F terms (F eps max |Y|,
                          rmsf_cases) of coordinates known to big on either route:  |sum_f proj_fj| <= sum_f pb_fj + F (F eps max |Y| + 2 big) sum_a |V_ja|
      (1 / F) sum_f proj_fj^2 = lambda_j for the unit eigenvectors of numpy.linalg.eigh(cov):  |v|^T B |v| + (1 / F) sum_f (2 |proj| pb + pb^2) and the
                          residual of LAPACK's symmetric eigen-solver, 16 (3 m) eps lambda_max."""
    F, n, kind, m = case
    c = fc.shape_case(*case)
    X, _, P, idx = measured(c)
    s = topology(c["N"])
    k = min(3 * m, 24)
    got = ctx.pca(s, c["frames"], fit=c["sel"], atoms=c["msel"], reference=0, n_modes=k)
    w, v = np.linalg.eigh(got["covariance"])
    assert np.array_equal(got["eigenvalues"], w[::-1]) and np.array_equal(got["modes"], cc.fix_signs(v[:, ::-1][:, :k].T))
    assert np.allclose(got["explained"], w[::-1][:k] / np.trace(got["covariance"]), rtol=1e-14) and got["projections"].shape == (F, k)
    again = ctx.project(s, c["frames"], idx, got["mean"], got["modes"], got["transforms"])
    assert again.tobytes() == got["projections"].tobytes()
    big = 4.0 * EPS * max(np.abs(c["frames"]).max(), np.abs(got["transforms"][:, 9:]).max())
    want = cc.projection(P, got["transforms"], got["mean"], got["modes"], big)
    proj, pb, V = got["projections"], want["bound"], np.abs(got["modes"])
    note(cc.ratio_within(proj, want["proj"], pb, (case, "pca projections")), (case, "pca"), "proj")
    ymax = np.repeat(np.linalg.norm(want["D"].reshape(F, m, 3) + (got["mean"] - X[0].mean(0)), axis=2).max(0), 3)   # |Y| about the reference's fit centroid
    total = pb.sum(0) + F * ((F * EPS * ymax + 2.0 * big) * V).sum(1)
    assert (np.abs(proj.sum(0)) <= total).all(), (case, "sum of projections", np.abs(proj.sum(0)).max(), total.min())
    B = cc.second_moments(want["D"], np.full((F, m), 2.0 * big))["cov_bound"]
    lam = got["eigenvalues"][:k]
    bound = np.einsum("ja,ab,jb->j", V, B, V) + (2.0 * np.abs(proj) * pb + pb * pb).mean(0) + 16.0 * 3 * m * EPS * lam[0]
    assert (np.abs((proj ** 2).mean(0) - lam) <= bound).all(), (case, "variance along the modes", float(np.abs((proj ** 2).mean(0) - lam).max()), float(bound.min()))
    # the modes are principal: numpy's own covariance of numpy's superposition has the same leading eigenvalues within the entry bounds (Weyl: 3 m max |E|)
    ref = cc.reference(case)
    assert (np.abs(np.linalg.eigvalsh(ref["cov"])[::-1][:k] - lam) <= 3 * m * ref["cov_bound"].max() + 16.0 * 3 * m * EPS * lam[0]).all(), (case, "eigenvalues")


# ---- capacity ------------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity(ctx):
    case = (33, 20, "disjoint", 65)
    c = fc.shape_case(*case)
    s, frames, sel, msel = topology(c["N"]), c["frames"], c["sel"], c["msel"]
    both = cc.capacity_bytes(33, 20, 65, True, True, True)
    only_dccm = cc.capacity_bytes(33, 20, 65, True, False, True)
    assert only_dccm < both
    aa.debug_set("rmsd_cap_bytes", both - 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        ctx.covariance(s, frames, fit=sel, atoms=msel, reference=0, cov=True, dccm=True)
    msg = str(e.value)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and msg.startswith("covariance: ") and "33 frames (F)" in msg and "65 measured atoms (m)" in msg
    assert f"{both} bytes" in msg and "rmsd_cap_bytes" in msg
    assert ctx.dccm(s, frames, fit=sel, atoms=msel, reference=0)["dccm"].shape == (65, 65)       # the smaller request still runs
    assert len(ctx.rmsf(s, frames, fit=sel, atoms=msel, reference=0)["rmsf"]) == 65             # as does arp_rmsf
    aa.debug_set("rmsd_cap_bytes", both)
    assert ctx.covariance(s, frames, fit=sel, atoms=msel, reference=0, cov=True, dccm=True)["covariance"].shape == (195, 195)
    aa.debug_set("rmsd_cap_bytes", only_dccm - 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        ctx.dccm(s, frames, fit=sel, atoms=msel, reference=0)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and f"{only_dccm} bytes" in str(e.value)
    aa.debug_set("rmsd_cap_bytes", 2048)
    with pytest.raises(aa.ArpeggiaError) as e:
        ctx.project(s, frames, msel, np.zeros((65, 3)), np.ones((3, 195)))
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "33 frames (F)" in str(e.value) and "3 modes (k)" in str(e.value)


def test_neither_output_is_refused(ctx):
    import ctypes as C

    c = fc.shape_case(5, 5, "same", 5)
    s = topology(c["N"])
    args, keep = aa.api._rmsd_args(s, c["frames"], c["sel"], "", "covariance")
    mean, rmsf, frame = np.zeros((5, 3), "<f8"), np.zeros(5, "<f4"), np.zeros(5, "<f4")
    rounds, last = C.c_uint32(), C.c_double()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    st = _lib.lib.arp_covariance(ctx._h, *args, None, 0, None, 0, 1, C.c_double(0.0), None, None, mean.ctypes.data_as(dp), rmsf.ctypes.data_as(fp), frame.ctypes.data_as(fp), None,
                                 C.byref(rounds), C.byref(last))
    assert st == _lib.ARP_ERR_BAD_INPUT and "neither cov nor dccm" in _lib.lib.arp_last_error().decode()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_1ubq(ctx, ubq_path):
    s = aa.Structure.load(ubq_path)
    frames = ts.jitter(rc.ubq_xyz(), 21, seed=11)
    sel = rc.ubq_selection("ca")
    got = aa.get_pca(s, frames, fit="ca", n_modes=10)
    assert np.array_equal(got["atom"], sel) and got["covariance"].shape == (228, 228) and got["modes"].shape == (10, 228) and got["projections"].shape == (21, 10)
    ref = cc.reference_of(frames[:, sel], max_rounds=50, tol=1e-4)
    assert ref["base"]["gap_ratio"] >= fc.MIN_GAP and got["n_rounds"] == ref["base"]["n_rounds"] and got["converged"]
    note(cc.assert_within(got, ref, "1ubq"), "1ubq", "iterated")
    check_own_outputs(got, 21, 76, "1ubq", ref["cov_bound"])
    assert (np.diff(got["eigenvalues"]) <= 0).all() and abs(got["explained"].sum() - got["eigenvalues"][:10].sum() / np.trace(got["covariance"])) < 1e-12
    assert 0.0 < got["cumulative"][-1] <= 1.0 + 1e-12 and (np.diff(got["cumulative"]) >= 0).all()
    d = aa.get_dccm(s, frames, fit="ca")
    note(cc.assert_within(d, ref, "1ubq dccm"), "1ubq dccm", "iterated")
    assert d["dccm"].tobytes() == aa.get_covariance(s, frames, fit="ca", cov=True, dccm=True)["dccm"].tobytes()
    names = lambda t: list(getattr(t, "column_names", None) or t.columns)   # (a pyarrow.Table, or a polars.DataFrame where polars is installed)
    table = aa.dccm_table(s, d)
    assert names(table) == aa.DCCM_COLUMNS and len(table) == 76 * 75 // 2
    one = aa.get_covariance(s, dccm=True)   # the file's one model is the one frame: nothing moves
    assert (one["covariance"] == 0).all() and (one["dccm"] == np.eye(76, dtype=np.float32)).all()


def test_models_are_the_frames_and_the_command_line(ctx, tmp_path):
    import synth
    from arpeggia_amd.__main__ import main

    ca = np.round(fc.ubq_ensemble(9, 0.5, 7), 3)   # 1ubq CA, nine models (what a PDB file's columns hold)
    N = ca.shape[1]
    s = topology(N, ca)
    got = aa.get_pca(s, fit="all", n_modes=4)
    same_bytes(got, aa.get_pca(topology(N), ca, fit="all", n_modes=4), "models and array", ("covariance", "projections", "modes") + RMSF_KEYS)
    path = tmp_path / "models.pdb"
    synth.write_pdb(atom_records(N, ca), path)
    loaded = aa.Structure.load(str(path))
    assert main(["dccm", "-i", str(path), "--fit", "all", "--matrix", str(tmp_path / "dccm.npy"), "-o", str(tmp_path / "out")]) == 0
    want = aa.get_dccm(loaded, fit="all")
    assert np.load(tmp_path / "dccm.npy").tobytes() == want["dccm"].tobytes()
    lines = (tmp_path / "out" / "dccm.csv").read_text().splitlines()
    assert lines[0].replace('"', "") == ",".join(aa.DCCM_COLUMNS) and len(lines) == 1 + N * (N - 1) // 2
    assert np.float32(lines[1].split(",")[-1]) == want["dccm"][0, 1]
    assert main(["pca", "-i", str(path), "--fit", "all", "--modes", "4", "--eigenvalues", str(tmp_path / "eig.csv"), "--modes-file", str(tmp_path / "modes.npy"),
                 "--projections", str(tmp_path / "proj.csv"), "--covariance", str(tmp_path / "cov.npy")]) == 0
    want = aa.get_pca(loaded, fit="all", n_modes=4)
    assert np.load(tmp_path / "cov.npy").tobytes() == want["covariance"].tobytes() and np.load(tmp_path / "modes.npy").tobytes() == want["modes"].tobytes()
    eig = (tmp_path / "eig.csv").read_text().splitlines()
    assert eig[0] == "mode,eigenvalue,explained,cumulative" and len(eig) == 5 and float(eig[1].split(",")[1]) == float(want["eigenvalues"][0])
    proj = (tmp_path / "proj.csv").read_text().splitlines()
    assert proj[0] == "frame,pc1,pc2,pc3,pc4" and len(proj) == 10 and [float(v) for v in proj[9].split(",")[1:]] == [float(v) for v in want["projections"][8]]
    assert main(["dccm", "-i", str(path)]) == 1   # nothing to write


def test_worst_ratio_is_reported(ctx):
    """Runs last: the largest error / bound ratios of the device over every case above (profiles/ records them)."""
    print(f"largest device error / bound: cov and dccm, one round {WORST['cov']:.4f} at {WORST['cov_what']}; iterated {WORST['iterated']:.4f} at {WORST['iterated_what']}; "
          f"projection {WORST['proj']:.4f} at {WORST['proj_what']}")
    assert WORST["cov"] <= 1.0 and WORST["iterated"] <= 1.0 and WORST["proj"] <= 1.0
