"""Covariance, DCCM and projection: everything that needs no device.  arp_covariance_host and arp_project_host (the definitions in plain sequential C++, the
yardsticks of k_cov_gram / k_cov_finish / k_dccm_finish / k_project) against the numpy reference on every shape and on the closed-form fixture, within the
derived bounds of tests/cov_cases.py; the cases' reach; every input check of the four calls, through ctx == NULL for the device calls; the capacity
arithmetic; the Python layer's argument checks; the sign convention of the modes and the explained variance; the exports and the CLI's flags."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import cov_cases as cc
import rmsf_cases as fc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib

WORST = {"cov": 0.0, "proj": 0.0, "what": None}
IDS = lambda s: f"F{s[0]}-n{s[1]}-{s[2]}-m{s[3]}"


def refused(status: int, fn, *args, match: str | None = None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)
    return str(e.value)


def test_exported():
    header = (Path(aa.__file__).resolve().parent.parent / "include" / "arpeggia_amd.h").read_text()
    for name in ("arp_covariance", "arp_project", "arp_covariance_host", "arp_project_host"):
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\(", header), name
    assert lib.arp_api_version() == 2  # additive exports do not move the layout version
    for word in ("a = 3 i + k", "dccm[m][m]", "cov[3 m][3 m]", "never computed", "rmsd_cap_bytes", "modes V[k][3 m]", "No fit is repeated"):
        assert word in header, word
    for name in ("get_covariance", "get_dccm", "get_pca", "get_projection", "covariance", "dccm", "pca", "covariance_host", "project_host", "dccm_table", "pca_modes"):
        assert callable(getattr(aa, name)), name
    for name in ("covariance", "dccm", "project", "pca"):
        assert callable(getattr(aa.Context, name)), name
    assert aa.DCCM_COLUMNS[-1] == "correlation" and aa.DCCM_COLUMNS[0] == "from_chain" and "to_atomi" in aa.DCCM_COLUMNS


def test_cases_reach_their_mechanisms():
    got = cc.check_shape_reach()
    print(f"shapes compared through R: {len(got['through_R'])}; on invariants only (n <= 2): {got['invariants_only']}")
    cc.check_closed_form_reach()
    cc.rigid_bound()
    assert cc.slab_plan(300, 3 * 260) == (80, 4) and cc.slab_plan(300, 260) == (64, 5) and cc.slab_plan(10000, 228) == (352, 29) and cc.slab_plan(1, 12) == (64, 1)


def test_reference_by_hand():
    """Two atoms outside a rigid fit, one moving +-1 along x and the other -+2 along x: cov by hand, dccm -1."""
    t = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0], [0, 0, 3.0]])
    XM = np.array([[[10.0, 0, 0], [0, 10.0, 0]], [[12.0, 0, 0], [-4.0, 10.0, 0]]])
    r = cc.reference_of(np.stack([t, t]), XM)
    want = np.zeros((6, 6))
    want[0, 0], want[3, 3], want[0, 3], want[3, 0] = 1.0, 4.0, -2.0, -2.0
    assert np.abs(r["cov"] - want).max() < 1e-13 and np.abs(r["dccm"] - [[1.0, -1.0], [-1.0, 1.0]]).max() < 1e-13
    assert np.abs(r["v"] - [1.0, 4.0]).max() < 1e-13
    assert np.array_equal(cc.dccm_of(np.array([[0.0, 0.0], [0.0, 2.0]])), [[1.0, 0.0], [0.0, 1.0]])   # an atom that does not move


# ---- the yardsticks against numpy ------------------------------------------------------------------------------------------------------------------------------
def host_bounds(ref: dict) -> dict:
    """arp_covariance_host fed numpy's own aligned and mean: its deviations differ from the reference's by the rounding of those absolute coordinates."""
    return cc.second_moments(ref["D"], np.full_like(ref["tau"], ref["base"]["big"]))


@pytest.mark.parametrize("case", cc.shapes(), ids=IDS)
def test_host_covariance_shapes(case):
    F, n, kind, m = case
    ref = cc.reference(case)
    got = aa.covariance_host(ref["base"]["aligned"], ref["base"]["mean"], cov=True, dccm=True)
    cc.check_matrices(got, m, case)
    b = host_bounds(ref)
    if cc.cov_only(case):
        assert (got["covariance"] == 0).all() and (got["dccm"] == np.eye(m, dtype=np.float32)).all()
        return
    ratio = cc.assert_within(got, dict(ref, cov_bound=b["cov_bound"], dccm_bound=b["dccm_bound"]), case)
    if ratio > WORST["cov"]:
        WORST.update(cov=ratio, what=case)
    only = aa.covariance_host(ref["base"]["aligned"], ref["base"]["mean"], cov=False, dccm=True)
    assert "covariance" not in only and only["dccm"].tobytes() == got["dccm"].tobytes()
    trace = np.diag(got["covariance"]).reshape(m, 3).sum(1)
    assert (np.abs(trace - ref["base"]["rmsf"] ** 2) <= b["v_bound"]).all(), (case, "block traces")


@pytest.mark.parametrize("case", cc.shapes(), ids=IDS)
def test_host_projection_shapes(case):
    F, n, kind, m = case
    c = fc.shape_case(*case)
    base = cc.reference(case)["base"]
    P = c["frames"][:, c["sel"] if c["msel"] is None else c["msel"]]
    tr = np.concatenate([base["R"].reshape(F, 9), base["t"]], axis=1)
    for k in cc.mode_counts(m):
        V = cc.random_modes(m, k)
        want = cc.projection(P, tr, base["mean"], V, base["big"])
        got = aa.project_host(P, base["mean"], V, tr)
        assert got.shape == (F, k) and got.dtype == np.float64
        WORST["proj"] = max(WORST["proj"], cc.ratio_within(got, want["proj"], want["bound"], (case, k)))
    already = np.array(base["aligned"])
    want = cc.projection(already, None, base["mean"], V, base["big"])
    WORST["proj"] = max(WORST["proj"], cc.ratio_within(aa.project_host(already, base["mean"], V), want["proj"], want["bound"], (case, "identity")))
    if n > 2:
        assert (np.abs(want["D"] - cc.reference(case)["D"]) <= np.repeat(base["bound"]["aligned"] + base["bound"]["mean"][None], 3, axis=1)).all()   # the two routes to d


def test_host_closed_form():
    fx, b = cc.closed_form(), cc.closed_form_bounds()
    host = aa.rmsf_host(fx["frames"][:, fx["sel"]], fx["frames"][:, fx["msel"]], reference=fx["ref_xyz"][fx["sel"]])
    got = aa.covariance_host(host["aligned"], host["mean"], cov=True, dccm=True)
    cc.check_matrices(got, len(fx["msel"]), "closed form")
    ratio = cc.assert_within(got, dict(cov=fx["cov"], dccm=fx["dccm"], cov_bound=b["cov_bound"], dccm_bound=b["dccm_bound"]), "closed form")
    print(f"closed form: largest host error / bound {ratio:.4f}; largest bounds cov {b['cov_bound'].max():.2e}, dccm {b['dccm_bound'].max():.2e}")
    assert set(np.unique(np.round(got["dccm"].astype(np.float64), 5))) == {-1.0, 0.0, 1.0}


def test_host_closed_form_projection():
    """The unit modes return the deviations themselves, which the fixture knows in closed form: no numerical reference."""
    fx, want = cc.closed_form(), cc.closed_form_projection()
    host = aa.rmsf_host(fx["frames"][:, fx["sel"]], fx["frames"][:, fx["msel"]], reference=fx["ref_xyz"][fx["sel"]])
    got = aa.project_host(fx["frames"][:, fx["msel"]], host["mean"], want["modes"], host["transforms"])
    WORST["proj"] = max(WORST["proj"], cc.ratio_within(got, want["proj"], want["bound"], "closed form"))
    again = aa.project_host(host["aligned"], host["mean"], want["modes"])
    cc.ratio_within(again, want["proj"], want["bound"], "closed form, superposed frames")


def test_host_rigid_shape_does_not_move():
    X, b = cc.rigid_case(), cc.rigid_bound()
    host = aa.rmsf_host(X)
    got = aa.covariance_host(host["aligned"], host["mean"])
    assert (np.abs(got["covariance"]) <= b["cov_bound"]).all(), float(np.abs(got["covariance"]).max())


def test_host_worst_ratio_is_reported():
    print(f"largest host error / bound: cov and dccm {WORST['cov']:.4f} at {WORST['what']}; projection {WORST['proj']:.4f}")
    assert WORST["cov"] <= 1.0 and WORST["proj"] <= 1.0


# ---- the refusals of the yardsticks ------------------------------------------------------------------------------------------------------------------------------
def test_host_refusals():
    a, mu = np.zeros((2, 3, 3)), np.zeros((3, 3))
    refused(_lib.ARP_ERR_BAD_INPUT, aa.covariance_host, np.zeros((0, 3, 3)), mu, match="at least one frame")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.covariance_host, np.zeros((2, 0, 3)), np.zeros((0, 3)), match="measured selection is empty")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.covariance_host, a, mu, cov=False, dccm=False, match="neither cov nor dccm")
    bad = a.copy()
    bad[1, 2, 0] = np.nan
    refused(_lib.ARP_ERR_BAD_INPUT, aa.covariance_host, bad, mu, match="frame 1, atom 2")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.covariance_host, a, bad[1], match="mean, atom 2")
    for args in ((np.zeros((2, 3)), mu), (a, np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            aa.covariance_host(*args)
    V = np.ones((2, 9))
    refused(_lib.ARP_ERR_BAD_INPUT, aa.project_host, np.zeros((0, 3, 3)), mu, V, match="at least one frame")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.project_host, np.zeros((2, 0, 3)), np.zeros((0, 3)), np.zeros((1, 0)), match="measured selection is empty")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.project_host, a, mu, np.zeros((0, 9)), match="k == 0")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.project_host, a, mu, np.ones((10, 9)), match="k = 10 modes")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.project_host, bad, mu, V, match="frame 1, atom 2")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.project_host, a, bad[1], V, match="mean, atom 2")
    Vb = V.copy()
    Vb[1, 4] = np.inf
    refused(_lib.ARP_ERR_BAD_INPUT, aa.project_host, a, mu, Vb, match="mode 1")
    tr = np.zeros((2, 12))
    tr[1, 3] = np.nan
    refused(_lib.ARP_ERR_BAD_INPUT, aa.project_host, a, mu, V, tr, match="transform of frame 1")
    for args in ((a, np.zeros((2, 3)), V), (a, mu, np.ones((2, 8))), (a, mu, np.ones(9)), (a, mu, V, np.zeros((3, 12))), (a, mu, V, np.zeros((2, 9)))):
        with pytest.raises(ValueError):
            aa.project_host(*args)


# ---- what arp_covariance and arp_project decide before the device is touched ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


def frames_of(s: aa.Structure, F: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)[None].repeat(F, 0)


def u32(a):
    a = np.ascontiguousarray(a, "<u4")
    return (a if len(a) else np.zeros(1, "<u4")).ctypes.data_as(C.POINTER(C.c_uint32)), a


def raw_cov(s, frames, sel, msel=None, ref=None, ref_frame=0, max_rounds=1, tol=0.0, call="arp_covariance") -> tuple:
    """arp_covariance (or arp_rmsf) with ctx == NULL: (status, message)."""
    n_frames, ptr, keep = aa.api._frames_arg(s, frames, "covariance")
    sp, sk = u32(sel)
    mp, mk = (None, None) if msel is None else u32(msel)
    rk = None if ref is None else np.ascontiguousarray(ref, "<f8")
    st = getattr(lib, call)(None, s._h, int(n_frames), ptr, sp, len(sk), mp, 0 if mk is None else len(mk), None if rk is None else rk.ctypes.data_as(C.POINTER(C.c_double)),
                            int(ref_frame), int(max_rounds), C.c_double(tol), *([None] * (8 if call == "arp_covariance" else 7)))
    return st, lib.arp_last_error().decode()


def raw_project(s, frames, msel, mean, modes, transforms=None) -> tuple:
    n_frames, ptr, keep = aa.api._frames_arg(s, frames, "project")
    mp, mk = u32(msel)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, "<f8").ctypes.data_as(C.POINTER(C.c_double))
    keepalive = [np.ascontiguousarray(a, "<f8") for a in (mean, modes) + ((transforms,) if transforms is not None else ())]
    st = lib.arp_project(None, s._h, int(n_frames), ptr, mp, len(mk), None if transforms is None else keepalive[2].ctypes.data_as(C.POINTER(C.c_double)),
                         keepalive[0].ctypes.data_as(C.POINTER(C.c_double)), keepalive[1].ctypes.data_as(C.POINTER(C.c_double)), len(np.atleast_2d(modes)) if np.size(modes) else 0, None)
    return st, lib.arp_last_error().decode()


def test_null_context_runs_only_the_checks(ubq):
    f = frames_of(ubq, 3)
    assert raw_cov(ubq, f, [0, 5, 9])[0] == _lib.ARP_OK          # (without a context even cov == dccm == NULL passes: nothing is computed)
    assert raw_cov(ubq, None, [0])[0] == _lib.ARP_OK
    assert raw_cov(ubq, f, [1, 2], msel=[0, 1, 7], ref_frame=2, max_rounds=50, tol=1e-4)[0] == _lib.ARP_OK
    assert raw_project(ubq, f, [0, 4], np.zeros((2, 3)), np.ones((6, 6)))[0] == _lib.ARP_OK
    assert raw_project(ubq, None, [3], np.zeros((1, 3)), np.ones((1, 3)), np.zeros((1, 12)))[0] == _lib.ARP_OK


def test_covariance_checks_are_those_of_rmsf_under_its_own_prefix(ubq):
    f = frames_of(ubq, 3)
    N = f.shape[1]
    ref = f[0].copy()
    ref[11, 2] = np.inf
    bad = f.copy()
    bad[2, 17, 1] = np.nan
    cases = [dict(sel=[]), dict(sel=[0, N]), dict(sel=[3, 3]), dict(sel=[0, 1], msel=[]), dict(sel=[0, 1], msel=[0, N]), dict(sel=[0, 1], msel=[5, 4]),
             dict(sel=[0, 1], max_rounds=0), dict(sel=[0, 1], tol=-1e-9), dict(sel=[0, 1], tol=float("nan")), dict(sel=[0, 1], ref_frame=3), dict(sel=[0, 1], ref=ref),
             dict(frames=bad, sel=[0, 1]), dict(frames=frames_of(ubq, 0), sel=[0, 1])]
    for kw in cases:
        frames = kw.pop("frames", f)
        st, msg = raw_cov(ubq, frames, **kw)
        st_r, msg_r = raw_cov(ubq, frames, call="arp_rmsf", **kw)
        assert st == st_r == _lib.ARP_ERR_BAD_INPUT, (kw, msg)
        assert msg == (("covariance" + msg_r[4:]) if msg_r.startswith("rmsf: ") else msg_r), (kw, msg, msg_r)
    assert raw_cov(ubq, f, [], msel=[])[1].startswith("covariance: ")


def test_project_checks(ubq):
    f = frames_of(ubq, 2)
    N = f.shape[1]
    mu, V = np.zeros((2, 3)), np.ones((2, 6))
    for msel, words in (([], "selection is empty"), ([0, N], "not an atom of the topology"), ([5, 4], "not strictly increasing")):
        m = max(len(msel), 1)
        st, msg = raw_project(ubq, f, msel, np.zeros((m, 3)), np.ones((1, 3 * m)))
        assert st == _lib.ARP_ERR_BAD_INPUT and words in msg and msg.startswith("project: "), (msel, msg)
    st, msg = raw_project(ubq, f, [0, 1], mu, np.zeros((0, 6)))
    assert st == _lib.ARP_ERR_BAD_INPUT and "k == 0" in msg
    st, msg = raw_project(ubq, f, [0, 1], mu, np.ones((7, 6)))
    assert st == _lib.ARP_ERR_BAD_INPUT and "k = 7 modes are more than the 6 coordinates of 2 measured atoms" in msg
    for which, words in (("mean", "mean, atom 1"), ("modes", "mode 1"), ("transforms", "transform of frame 1")):
        arrays = {"mean": mu.copy(), "modes": V.copy(), "transforms": np.zeros((2, 12))}
        arrays[which][1, 1] = np.nan
        st, msg = raw_project(ubq, f, [0, 1], arrays["mean"], arrays["modes"], arrays["transforms"])
        assert st == _lib.ARP_ERR_BAD_INPUT and words in msg, (which, msg)
    bad = f.copy()
    bad[1, 17, 1] = np.nan
    st, msg = raw_project(ubq, bad, [0, 1], mu, V)
    assert st == _lib.ARP_ERR_BAD_INPUT and "frame 1, atom 17" in msg


def test_input_errors_come_before_the_missing_device(ubq):
    """Whatever the machine: a bad input is ARP_ERR_BAD_INPUT (or a ValueError of the Python layer) from every layer, never ARP_ERR_NO_DEVICE."""
    f = frames_of(ubq, 2)
    for fn in (aa.get_covariance, aa.get_dccm, aa.get_pca):
        refused(_lib.ARP_ERR_BAD_INPUT, fn, ubq, f, fit="ca", chains="Z", match="covariance: the selection is empty")
        refused(_lib.ARP_ERR_BAD_INPUT, fn, ubq, f, atoms=np.zeros(0, np.int64), match="measured selection is empty")
        refused(_lib.ARP_ERR_BAD_INPUT, fn, ubq, f, max_rounds=0, match="max_rounds")
        refused(_lib.ARP_ERR_BAD_INPUT, fn, ubq, f, tol=-1.0, match="tol")
        refused(_lib.ARP_ERR_BAD_INPUT, fn, ubq, f, reference=2, match="ref_frame 2")
        refused(_lib.ARP_ERR_BAD_INPUT, fn, ubq, np.zeros((2, 5, 3)), match="shape")
        for kw in (dict(reference="median"), dict(reference=-1), dict(fit="sidechain")):
            with pytest.raises(ValueError):
                fn(ubq, f, **kw)
    with pytest.raises(ValueError):
        aa.get_covariance(ubq, f, cov=False, dccm=False)
    for n_modes in (0, -1, 2.5):
        with pytest.raises(ValueError):
            aa.get_pca(ubq, f, n_modes=n_modes)
    m = 76
    mu, V = np.zeros((m, 3)), np.ones((2, 3 * m))
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_projection, ubq, f, "ca", mu, np.zeros((0, 3 * m)), match="k == 0")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_projection, ubq, np.zeros((2, 5, 3)), "ca", mu, V, match="shape")
    for args in ((np.zeros((m - 1, 3)), V), (mu, np.ones((2, 3 * m - 1))), (mu, V, np.zeros((3, 12)))):
        with pytest.raises(ValueError):
            aa.get_projection(ubq, f, "ca", *args)


def test_capacity_arithmetic():
    """cov_cases.capacity_bytes by hand on one shape: F = 33, n = 64, m = 65 (m_pad = 68) with a measured set of its own."""
    resident = 33 * 3 * 64 * 8 + 33 * 8 + 33 * 3 * 68 * 8
    dev = 33 * 3 * 68 * 8
    tiles = lambda L: -(-L // 32) * (-(-L // 32) + 1) // 2
    assert cc.slab_plan(33, 204) == (64, 1) and cc.slab_plan(33, 68) == (64, 1) and tiles(204) == 28 and tiles(68) == 6
    assert cc.capacity_bytes(33, 64, 65, True, True, False) == resident + dev + 204 * 204 * 8 + 28 * 1024 * 8
    assert cc.capacity_bytes(33, 64, 65, True, False, True) == resident + dev + 68 * 68 * 4 + 6 * 1024 * 8
    assert cc.capacity_bytes(33, 64, 65, True, True, True) == resident + dev + 204 * 204 * 8 + 68 * 68 * 4 + 28 * 1024 * 8
    assert cc.capacity_bytes(33, 64, 64, False, True, False) == 33 * 3 * 64 * 8 + 33 * 8 + 33 * 3 * 64 * 8 + 192 * 192 * 8 + 21 * 1024 * 8


# ---- the host half of pca ----------------------------------------------------------------------------------------------------------------------------------------
def test_mode_signs_and_explained_variance():
    rng = np.random.default_rng(3)
    D = rng.normal(size=(40, 12)) * np.array([5.0, 3.0, 2.0] + [0.5] * 9)
    c = D.T @ D / 40
    got = aa.pca_modes(c, 4)
    w, v = np.linalg.eigh(c)
    assert np.array_equal(got["eigenvalues"], w[::-1]) and got["modes"].shape == (4, 12) and (np.diff(got["eigenvalues"]) <= 0).all()
    assert np.array_equal(got["modes"], cc.fix_signs(v[:, ::-1][:, :4].T))
    for row in got["modes"]:
        assert row[int(np.argmax(np.abs(row)))] > 0 and abs(np.linalg.norm(row) - 1.0) < 1e-14
    assert np.allclose(got["explained"], w[::-1][:4] / np.trace(c), rtol=1e-15) and np.allclose(got["cumulative"], np.cumsum(got["explained"]), rtol=1e-15)
    full = aa.pca_modes(c, 100)                        # n_modes is capped at the coordinates
    assert full["modes"].shape == (12, 12) and abs(full["cumulative"][-1] - 1.0) < 1e-14 and abs(full["explained"].sum() - w.sum() / np.trace(c)) < 1e-14
    tie = aa.pca_modes(np.diag([2.0, 1.0, 1.0]) + 0.0, 1)
    assert tie["modes"].tolist() == [[1.0, 0.0, 0.0]]
    assert cc.fix_signs(np.array([[-0.5, 0.5, 0.1], [0.5, -0.5, 0.1]])).tolist() == [[0.5, -0.5, -0.1], [0.5, -0.5, 0.1]]   # the lowest index on ties
    zero = aa.pca_modes(np.zeros((3, 3)), 2)
    assert (zero["explained"] == 0).all() and (zero["cumulative"] == 0).all()
    for bad in (np.zeros((2, 3)), np.zeros(4), np.zeros((0, 0))):
        with pytest.raises(ValueError):
            aa.pca_modes(bad)


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_defaults_and_flags(tmp_path):
    from arpeggia_amd.__main__ import build_parser

    p = build_parser()
    a = p.parse_args(["dccm", "-i", "x.pdb", "--matrix", "m.npy"])
    assert a.fit == "ca" and a.atoms is None and a.chains == "" and a.reference == "mean" and a.max_rounds == 50 and a.tol == 1e-4 and str(a.matrix) == "m.npy"
    assert a.output is None and a.filename == "dccm" and a.output_format == "csv"
    a = p.parse_args(["dccm", "-i", "x.pdb", "-o", str(tmp_path), "-f", "pairs", "-t", "parquet", "--fit", "backbone", "--atoms", "heavy", "-c", "A,B", "--reference", "3",
                      "--max-rounds", "7", "--tol", "0.01"])
    assert a.fit == "backbone" and a.atoms == "heavy" and a.chains == "A,B" and a.reference == 3 and a.max_rounds == 7 and a.tol == 0.01
    assert a.filename == "pairs" and a.output_format == "parquet" and a.matrix is None
    a = p.parse_args(["pca", "-i", "x.pdb"])
    assert a.modes == 10 and a.eigenvalues is None and a.modes_file is None and a.projections is None and a.covariance is None and a.reference == "mean"
    a = p.parse_args(["pca", "-i", "x.pdb", "--modes", "3", "--eigenvalues", "e.csv", "--modes-file", "v.npy", "--projections", "p.csv", "--covariance", "c.npy", "--fit", "all"])
    assert a.modes == 3 and str(a.eigenvalues) == "e.csv" and str(a.modes_file) == "v.npy" and str(a.projections) == "p.csv" and str(a.covariance) == "c.npy" and a.fit == "all"
    for argv in (["dccm", "--matrix", "m.npy"], ["dccm", "-i", "x.pdb", "--fit", "sidechain"], ["pca", "-i", "x.pdb", "--reference", "median"], ["pca", "-i", "x.pdb", "--modes", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    from arpeggia_amd.__main__ import main

    assert main(["dccm", "-i", str(tmp_path / "missing.pdb"), "--matrix", str(tmp_path / "m.npy")]) == 1
