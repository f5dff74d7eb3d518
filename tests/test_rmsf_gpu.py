"""RMSF and the mean structure (arp_rmsf) on the device.

k_rmsd_pack<measured> / k_rmsf_fit / k_rmsf_sweep / k_rmsf_mean_finish / k_rmsf_change / k_rmsf_dev_finish / k_rmsf_frame / k_rmsf_aligned at every lane, tile,
slab and workgroup edge of tests/rmsf_cases.py: one round within the derived bounds of numpy and of arp_rmsf_host; proper rotations; aligned = R x + t; the
superposition optimal by the rmsd call's own value, on every case including those whose top eigenvalue is double; the identities between the outputs; the
iterated mean with numpy's number of rounds; identical bytes from call to call and from pass size to pass size; the capacity error; 1ubq end to end.
Expected values never come from the call under test, except where bit-equality between two calls is the property.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import rmsd_cases as rc
import rmsf_cases as fc
import trajectory_shapes as ts
from arpeggia_amd import _lib

pytestmark = pytest.mark.gpu

KNOBS = ("rmsd_chunk_atoms", "rmsd_cap_bytes")
WORST = {"ratio": 0.0, "what": None, "iterated": 0.0, "iterated_what": None}   # the largest error / bound of the device (printed by the last test)
OUTPUTS = ("mean", "rmsf", "frame_rmsd", "aligned", "transforms")


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


def embed(X: np.ndarray) -> dict:
    """A case of its own from [F, n, 3] fit coordinates: the n atoms among N = n + 2, with two decoys the selection skips."""
    F, n = X.shape[:2]
    N, sel, _ = fc.layout(n, "same", n)
    frames = np.random.default_rng(n).normal(scale=100.0, size=(F, N, 3))
    frames[:, sel] = X
    return {"N": N, "sel": sel, "msel": None, "frames": frames}


def call(ctx, c: dict, reference=0, **kw) -> dict:
    return ctx.rmsf(topology(c["N"]), c["frames"], fit=c["sel"], atoms=c["msel"], reference=reference, aligned=True, transforms=True, **kw)


def iterate_from(ctx, c: dict, ref_frame: int, max_rounds: int, tol: float) -> dict:
    """arp_rmsf itself, iterating from frame ref_frame (the Python layer's reference="mean" starts from frame 0): rmsf, n_rounds, last_change."""
    import ctypes as C

    s = topology(c["N"])
    args, keep = aa.api._rmsd_args(s, c["frames"], c["sel"], "", "rmsf")
    F, n = c["frames"].shape[0], len(c["sel"])
    mean, rmsf, frame = np.zeros((n, 3), "<f8"), np.zeros(n, "<f4"), np.zeros(F, "<f4")
    rounds, last = C.c_uint32(), C.c_double()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    st = _lib.lib.arp_rmsf(ctx._h, *args, None, 0, None, ref_frame, max_rounds, C.c_double(tol), mean.ctypes.data_as(dp), rmsf.ctypes.data_as(fp), frame.ctypes.data_as(fp),
                           None, None, C.byref(rounds), C.byref(last))
    assert st == _lib.ARP_OK, _lib.lib.arp_last_error().decode()
    return {"mean": mean, "rmsf": rmsf, "frame_rmsd": frame, "n_rounds": int(rounds.value), "last_change": float(last.value)}


def same_bytes(a: dict, b: dict, what):
    for key in OUTPUTS:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)
    assert a["n_rounds"] == b["n_rounds"] and a["last_change"] == b["last_change"], what


def note(ratio: float, what, key="ratio"):
    if ratio > WORST[key]:
        WORST[key] = ratio
        WORST["what" if key == "ratio" else "iterated_what"] = what


def check_invariants(ctx, got: dict, c: dict, what, ref_frame: int = 0):
    """What holds whichever top eigenvector was chosen."""
    frames, sel = c["frames"], c["sel"]
    F, n = frames.shape[0], len(sel)
    same = c["msel"] is None
    X = frames[:, sel]
    measured = X if same else frames[:, c["msel"]]
    assert got["rmsf"].dtype == np.float32 and got["frame_rmsd"].dtype == np.float32 and got["bfactor"].dtype == np.float32
    assert got["mean"].shape == (measured.shape[1], 3) and got["aligned"].shape == measured.shape and got["transforms"].shape == (F, 12)
    assert np.array_equal(got["atom"], sel if same else c["msel"])
    fc.check_rotations(got["transforms"], what)
    R, t = got["transforms"][:, :9].reshape(F, 3, 3), got["transforms"][:, 9:]
    again = np.einsum("fab,fib->fia", R, measured) + t[:, None]
    size = max(np.abs(measured).max(), np.abs(t).max())
    assert np.abs(again - got["aligned"]).max() <= 8.0 * fc.EPS * size, (what, "aligned = R x + t", np.abs(again - got["aligned"]).max(), size)
    # optimal without numpy's SVD: the plain rmsd of the superposed fit atoms to the reference's is the rmsd call's value, within that call's bound
    fit_aligned = got["aligned"] if same else np.einsum("fab,fib->fia", R, X) + t[:, None]
    there = max(np.abs(fit_aligned).max(), np.abs(X[ref_frame]).max())
    slack = 4.0 * fc.EPS * there + (0.0 if same else 8.0 * fc.EPS * max(np.abs(X).max(), np.abs(t).max()))
    best = ctx.rmsd(topology(c["N"]), frames, reference=ref_frame, atoms=sel).astype(np.float64)
    bound = rc.tolerance(best, rc.reference(X[ref_frame][None], X)["gsum"][0])
    plain = fc.plain_rmsd(fit_aligned, X[ref_frame])
    assert (np.abs(plain - best) <= bound + slack).all(), (what, "optimal", float(np.abs(plain - best).max()))
    if same:
        lhs, rhs = n * (got["frame_rmsd"].astype(np.float64) ** 2).sum(), F * (got["rmsf"].astype(np.float64) ** 2).sum()
        assert abs(lhs - rhs) <= 2.0 ** -22 * max(lhs, rhs), (what, lhs, rhs)   # each output is rounded to f32 once (2^-24), squared (2^-23), on either side
        assert np.linalg.norm(got["mean"].mean(0) - X[ref_frame].mean(0)) <= 8.0 * fc.EPS * there, (what, "centred mean")
    want_b = (8.0 * np.pi ** 2 / 3.0) * got["rmsf"].astype(np.float64) ** 2
    assert (np.abs(got["bfactor"] - want_b) <= 2.0 ** -23 * want_b).all(), (what, "bfactor")


def check_one_round(ctx, c: dict, what, passes: bool = False, through_r: bool = True) -> dict:
    got = call(ctx, c)
    assert got["n_rounds"] == 1 and got["converged"] == (got["last_change"] <= 1e-4)
    check_invariants(ctx, got, c, what)
    frames, sel = c["frames"], c["sel"]
    X, XM = frames[:, sel], None if c["msel"] is None else frames[:, c["msel"]]
    if through_r:
        ref = fc.reference(X, XM)
        note(fc.assert_within(got, ref, (what, "numpy")), what)
        host = aa.rmsf_host(X, XM)
        as_ref = dict(ref, mean=host["mean"], rmsf=host["rmsf"].astype(np.float64), frame_rmsd=host["frame_rmsd"].astype(np.float64), aligned=host["aligned"],
                      R=host["transforms"][:, :9].reshape(-1, 3, 3), t=host["transforms"][:, 9:])
        bound = dict(ref["bound"])
        for key in ("rmsf", "frame_rmsd"):   # both sides are rounded to f32 here
            bound[key] = bound[key] + 2.0 ** -23 * as_ref[key]
        fc.assert_within(got, dict(as_ref, bound=bound), (what, "host"))
    same_bytes(got, call(ctx, c), (what, "two calls"))
    if passes:
        F, N = frames.shape[:2]
        for per in sorted({F, -(-F // 2), 1}):   # 1, 2 and F passes
            aa.debug_set("rmsd_chunk_atoms", per * N)
            same_bytes(got, call(ctx, c), (what, "frames per pass", per))
        aa.debug_set("rmsd_chunk_atoms", 0)
    return got


# ---- one round on every shape ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.shapes(), ids=lambda s: f"F{s[0]}-n{s[1]}-{s[2]}-m{s[3]}")
def test_shapes(ctx, case):
    F, n, kind, m = case
    got = check_one_round(ctx, fc.shape_case(*case), case, passes=kind != "same" or n in (5, 65), through_r=n > 2)
    if n == 1 and kind == "same":
        assert (got["rmsf"] == 0).all() and (got["frame_rmsd"] == 0).all()


@pytest.mark.parametrize("name", sorted(rc.degenerate_cases()))
def test_degenerate_geometry(ctx, name):
    """The double top eigenvalues (collinear, n <= 2: invariants only), planar and mirror-image selections, one rigid shape tumbled and 1.6 10^5 A out."""
    X = rc.degenerate_cases()[name]
    c = embed(X)
    got = check_one_round(ctx, c, name, passes=True, through_r=name in fc.THROUGH_R)
    if name == "mirror":   # frames 1 and 3 are mirror images of the reference: they stay unsuperposed
        assert got["frame_rmsd"][1] > 1.0 and fc.plain_rmsd(got["aligned"], X[0])[[1, 3]].min() > 1.0 and fc.plain_rmsd(got["aligned"], X[0])[2] < 1e-6
    if name in ("tumble", "drift"):
        fc.assert_rigid(got, fc.reference(X), X[0], name)


def test_other_references(ctx):
    """A reference frame that is not the first, in another slab; a reference that is no frame."""
    c = fc.shape_case(33, 64, "disjoint", 65)
    X, XM = c["frames"][:, c["sel"]], c["frames"][:, c["msel"]]
    for k in (5, 32):
        got = call(ctx, c, reference=k)
        note(fc.assert_within(got, fc.reference(X, XM, ref=k), ("frame", k)), ("frame", k))
        check_invariants(ctx, got, c, ("frame", k), ref_frame=k)
    other = c["frames"][7] + np.random.default_rng(1).normal(scale=0.5, size=c["frames"][7].shape) + 40.0
    got = call(ctx, c, reference=other)
    note(fc.assert_within(got, fc.reference(X, XM, ref=other[c["sel"]]), "external"), "external")
    assert got["n_rounds"] == 1


# ---- the iterated mean ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.ITERATED))
def test_iterated_mean(ctx, name):
    fx = fc.iterated_fixture(name)
    X = np.array(fx["frames"])
    c = embed(X)
    got = call(ctx, c, reference="mean", max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"])
    ref = fc.reference(X, max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"])
    assert got["n_rounds"] == ref["n_rounds"] == fx["rounds"] and got["last_change"] <= fx["tol"] and got["converged"]
    assert abs(got["last_change"] - ref["last_change"]) <= 0.5 * ref["last_change"]
    ratio = fc.assert_within(got, ref, name)
    print(f"{name}: {got['n_rounds']} rounds, last change {got['last_change']:.3e}, largest error / iterated bound {ratio:.4f}")
    note(ratio, name, "iterated")
    fc.check_rotations(got["transforms"], name)
    same_bytes(got, call(ctx, c, reference="mean", max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"]), (name, "two calls"))
    # one more numpy round started from the device's mean moves it by no more than tol plus the one-round bound
    more = fc.reference(X, ref=got["mean"])
    assert more["last_change"] <= fx["tol"] + np.sqrt((more["bound"]["mean"] ** 2).mean()), (name, more["last_change"])
    # Started from the last frame instead of the first: both runs stop within tol / 9 (rms over the atoms) of the iteration's fixed point -- the changes
    # shrink tenfold per round -- so their rmsf differ, as an rms over the atoms, by less than tol, plus the iterated bound of either
    first = iterate_from(ctx, c, 0, fc.ITERATED_ROUNDS, fx["tol"])
    assert first["rmsf"].tobytes() == got["rmsf"].tobytes() and first["n_rounds"] == got["n_rounds"]   # (what reference="mean" is)
    back = iterate_from(ctx, c, len(X) - 1, fc.ITERATED_ROUNDS, fx["tol"])
    diff = back["rmsf"].astype(np.float64) - got["rmsf"]
    assert np.sqrt((diff ** 2).mean()) <= fx["tol"] + 2.0 * (ref["bound"]["rmsf"] * ref["scale"]).max(), (name, np.sqrt((diff ** 2).mean()))
    assert back["last_change"] <= fx["tol"]


def test_max_rounds_ends_the_call(ctx):
    c = embed(fc.cap_case())
    got = call(ctx, c, reference="mean", max_rounds=fc.ITERATED_ROUNDS, tol=fc.CAP_TOL)
    assert got["n_rounds"] == fc.ITERATED_ROUNDS and got["last_change"] > fc.CAP_TOL and not got["converged"]
    fc.check_rotations(got["transforms"], "cap")
    three = call(ctx, c, reference="mean", max_rounds=3, tol=0.0)
    assert three["n_rounds"] == 3 and three["last_change"] > 0.0
    ref = fc.reference(fc.cap_case(), max_rounds=3, tol=0.0)
    note(fc.assert_within(three, ref, "three rounds"), "three rounds", "iterated")


# ---- capacity ------------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity(ctx):
    c = fc.shape_case(33, 64, "disjoint", 65)
    s, frames, sel, msel = topology(c["N"]), c["frames"], c["sel"], c["msel"]
    packed = 33 * 3 * 64 * 8 + 33 * 8                      # X and G: what the rmsd calls keep resident
    need = packed + 33 * 3 * 68 * 8                        # and XM (m_pad = 68)
    aa.debug_set("rmsd_cap_bytes", need - 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        ctx.rmsf(s, frames, fit=sel, atoms=msel, reference=0)
    msg = str(e.value)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "33 frames (F)" in msg and "64 fit atoms (n)" in msg and "65 measured atoms (m)" in msg
    assert f"{need} bytes" in msg and "rmsd_cap_bytes" in msg
    assert len(ctx.rmsd(s, frames, atoms=sel)) == 33        # the rmsd calls still run at a cap where they did before
    assert len(ctx.rmsf(s, frames, fit=sel, reference=0)["rmsf"]) == 64   # as does the call without a measured set of its own
    aa.debug_set("rmsd_cap_bytes", need)
    assert len(ctx.rmsf(s, frames, fit=sel, atoms=msel, reference=0)["rmsf"]) == 65
    aa.debug_set("rmsd_cap_bytes", packed - 1)
    for fn in (lambda: ctx.rmsf(s, frames, fit=sel, reference=0), lambda: ctx.rmsd(s, frames, atoms=sel)):
        with pytest.raises(aa.ArpeggiaError) as e:
            fn()
        assert e.value.status == _lib.ARP_ERR_CAPACITY and f"{packed} bytes" in str(e.value)


def test_outputs_on_request(ctx):
    c = fc.shape_case(5, 65, "overlap", 63)
    s = topology(c["N"])
    full = call(ctx, c)
    bare = ctx.rmsf(s, c["frames"], fit=c["sel"], atoms=c["msel"], reference=0)
    assert "aligned" not in bare and "transforms" not in bare and "residue" not in bare
    for key in ("mean", "rmsf", "frame_rmsd", "bfactor"):
        assert bare[key].tobytes() == full[key].tobytes(), key
    one = ctx.rmsf(s, c["frames"], fit=c["sel"], atoms=c["msel"], reference=0, aligned=True)
    assert one["aligned"].tobytes() == full["aligned"].tobytes() and "transforms" not in one


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_1ubq(ctx, ubq_path):
    s = aa.Structure.load(ubq_path)
    frames = ts.jitter(rc.ubq_xyz(), 21, seed=11)
    sel, msel = rc.ubq_selection("ca"), rc.ubq_selection("heavy")
    got = aa.get_rmsf(s, frames, fit="ca", atoms="heavy", level="residue", aligned=True, transforms=True)
    assert np.array_equal(got["atom"], msel) and len(got["rmsf"]) == 602
    ref = fc.reference(frames[:, sel], frames[:, msel], max_rounds=50, tol=1e-4)
    assert ref["gap_ratio"] >= fc.MIN_GAP and not any(0.5e-4 < ch < 2e-4 for ch in ref["changes"])   # no change near the default tol
    assert got["n_rounds"] == ref["n_rounds"] and got["converged"]
    note(fc.assert_within(got, ref, "1ubq"), "1ubq", "iterated")
    assert 0.2 < float(np.median(got["rmsf"])) < 0.7          # 0.3 A of noise per coordinate: 0.3 sqrt(3) = 0.52 A, less what the fit takes up
    want_b = (8.0 * np.pi ** 2 / 3.0) * got["rmsf"].astype(np.float64) ** 2
    assert got["bfactor"].dtype == np.float32 and (np.abs(got["bfactor"] - want_b) <= 2.0 ** -23 * want_b).all()
    rows, value = fc.residue_rmsf(fc.ubq_residue_keys(msel), got["rmsf"])
    res = got["residue"]
    assert len(rows) == 76 == len(res["rmsf"]) and res["rmsf"].dtype == np.float32 and int(res["n_atoms"].sum()) == 602
    assert (np.abs(res["rmsf"] - value) <= 2.0 ** -23 * value).all()
    ref_rows, ref_value = fc.residue_rmsf(fc.ubq_residue_keys(msel), ref["rmsf"])
    assert (np.abs(res["rmsf"] - ref_value) <= 2.0 * (ref["bound"]["rmsf"] * ref["scale"]).max() + 2.0 ** -22 * ref_value).all()
    assert fc.ubq_residue_keys(res["atom"]) == rows
    same_bytes(got, ctx.rmsf(s, frames, fit=sel, atoms=msel, aligned=True, transforms=True), "1ubq, context and explicit indices")
    names = lambda t: list(getattr(t, "column_names", None) or t.columns)   # (a pyarrow.Table, or a polars.DataFrame where polars is installed)
    table = aa.rmsf_table(s, got, "residue")
    assert names(table) == aa.RMSF_RESIDUE_COLUMNS and len(table) == 76
    assert names(aa.rmsf_table(s, got)) == aa.RMSF_COLUMNS
    one = aa.get_rmsf(s)   # the file's one model is the one frame: nothing moves
    assert one["n_rounds"] == 1 and (one["rmsf"] == 0).all() and one["frame_rmsd"].tolist() == [0.0]


def test_models_are_the_frames_and_the_command_line(ctx, tmp_path):
    import synth
    from arpeggia_amd.__main__ import main

    c = fc.shape_case(5, 65, "same", 65)
    frames = np.round(np.array(c["frames"]) * 0.1, 3)   # (what a PDB file's columns hold)
    N = c["N"]
    s = topology(N, frames)
    kw = dict(fit=c["sel"], reference=0, aligned=True, transforms=True, level="residue")
    got = aa.get_rmsf(s, **kw)
    assert got["frame_rmsd"].shape == (5,)
    same_bytes(got, aa.get_rmsf(topology(N), frames, **kw), "models and array")
    note(fc.assert_within(got, fc.reference(frames[:, c["sel"]]), "models"), "models")
    path = tmp_path / "models.pdb"
    synth.write_pdb(atom_records(N, frames), path)
    assert main(["rmsf", "-i", str(path), "-o", str(tmp_path / "out"), "--fit", "all", "-l", "residue", "--frames", str(tmp_path / "frames.csv"), "--aligned",
                 str(tmp_path / "aligned.npy")]) == 0
    lines = (tmp_path / "out" / "rmsf.csv").read_text().splitlines()
    assert lines[0] == ",".join(aa.RMSF_RESIDUE_COLUMNS) and len(lines) == 1 + N
    everything = aa.get_rmsf(aa.Structure.load(str(path)), fit="all", aligned=True)
    assert [float(l.split(",")[-2]) for l in lines[1:]] == [float(v) for v in everything["rmsf"]]   # one atom per residue: the residue's value is the atom's
    assert (tmp_path / "frames.csv").read_text().splitlines()[0] == "frame,rmsd" and len((tmp_path / "frames.csv").read_text().splitlines()) == 6
    assert np.load(tmp_path / "aligned.npy").tobytes() == everything["aligned"].tobytes()
    assert main(["rmsf", "-i", str(path), "-o", str(tmp_path / "out"), "-f", "atoms", "--reference", "2"]) == 0
    atoms = (tmp_path / "out" / "atoms.csv").read_text().splitlines()
    assert atoms[0] == ",".join(aa.RMSF_COLUMNS) and len(atoms) == 1 + N


def test_worst_ratio_is_reported(ctx):
    """Runs last: the largest error / bound ratios of the device over every case above (profiles/ records them)."""
    print(f"largest device error / bound: one round {WORST['ratio']:.4f} at {WORST['what']}; iterated {WORST['iterated']:.4f} at {WORST['iterated_what']}")
    assert WORST["ratio"] <= 1.0 and WORST["iterated"] <= 1.0
