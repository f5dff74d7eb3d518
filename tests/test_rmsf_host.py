"""RMSF and the mean structure: everything that needs no device.  arp_rmsf_host (the definition in plain sequential C++, the yardstick of k_rmsf_fit /
k_rmsf_sweep / k_rmsf_frame) against the numpy reference on every case, within the derived bounds; the gap-0 cases on invariants; the iterated mean with
numpy's own number of rounds; every input check of arp_rmsf_host and of arp_rmsf with ctx == NULL; the cases' reach; the residue rows; the exports and the
CLI's flags."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import rmsd_cases as rc
import rmsf_cases as fc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib

WORST = {"ratio": 0.0, "what": None, "iterated": 0.0}


def refused(status: int, fn, *args, match: str | None = None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)
    return str(e.value)


def test_exported():
    header = (Path(aa.__file__).resolve().parent.parent / "include" / "arpeggia_amd.h").read_text()
    for name in ("arp_rmsf", "arp_rmsf_host"):
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\(", header), name
    assert lib.arp_api_version() == 2  # additive exports do not move the layout version
    for word in ("msel", "max_rounds", "last_change", "frame_rmsd", "transforms", "aligned", "lowest index on ties", "rmsd_cap_bytes", "E[y^2] - E[y]^2"):
        assert word in header, word
    for name in ("get_rmsf", "rmsf", "rmsf_host", "rmsf_residues", "rmsf_table"):
        assert callable(getattr(aa, name))
    assert callable(aa.Context.rmsf)
    assert aa.RMSF_COLUMNS[-2:] == ["rmsf", "bfactor"] and aa.RMSF_RESIDUE_COLUMNS[-2:] == ["rmsf", "bfactor"] and "n_atoms" in aa.RMSF_RESIDUE_COLUMNS


def test_cases_reach_their_mechanisms():
    got = fc.check_shape_reach()
    print(f"shapes compared through R: {len(got['through_R'])}; on invariants only (n <= 2): {got['invariants_only']}")
    ratios = fc.check_degenerate_reach()
    print("degenerate cases, gap / Gs:", {k: float(f"{v:.3g}") for k, v in ratios.items()}, "-- invariants only:", fc.INVARIANTS_ONLY)


def test_iterated_fixtures_converge_as_measured():
    """numpy's own sequences: strictly decreasing, ten times apart around each fixture's tol; the unrelated frames are still moving after 50 rounds."""
    for name, got in fc.check_iterated_reach().items():
        print(name, "changes", [float(f"{c:.2e}") for c in got["changes"]], "tol", f"{got['tol']:.2e}", "rounds", got["rounds"], "gap / Gs", f"{got['gap_ratio']:.3f}")
    print(f"cap case: change after {fc.ITERATED_ROUNDS} rounds {fc.check_cap_reach():.3e}")


def test_reference_by_hand():
    """The numpy reference itself on frames small enough to do by hand."""
    t = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0], [0, 0, 3.0]])
    turn = np.array([[0.0, -1, 0], [1.0, 0, 0], [0, 0, 1.0]])   # 90 degrees about z
    X = np.stack([t, t @ turn.T + 5.0, t - 2.0])
    r = fc.reference(X)
    assert r["rmsf"].max() < 1e-14 and r["frame_rmsd"].max() < 1e-14 and np.abs(r["mean"] - t).max() < 1e-14
    assert np.abs(r["R"][1] - turn.T).max() < 1e-14 and np.abs(r["aligned"] - t).max() < 1e-13
    # one atom displaced by 3 A along x in one of two frames that superpose otherwise: no, the fit moves too -- take the measured atom outside the fit
    XM = np.array([[[10.0, 0, 0]], [[13.0, 0, 0]]])
    r = fc.reference(np.stack([t, t]), XM)
    assert abs(r["rmsf"][0] - 1.5) < 1e-14 and np.abs(r["mean"][0] - [11.5, 0, 0]).max() < 1e-14
    # a mirror image stays unsuperposed
    m = fc.reference(np.stack([t, rc.mirror(t)]))
    assert m["frame_rmsd"].min() > 0.1 and abs(np.linalg.det(m["R"][1]) - 1.0) < 1e-14


# ---- arp_rmsf_host against numpy ---------------------------------------------------------------------------------------------------------------------------
def host_of(X, XM=None, ref=0, max_rounds=1, tol=0.0) -> dict:
    return aa.rmsf_host(X, XM, reference=ref, max_rounds=max_rounds, tol=tol)


def check_invariants(got: dict, X: np.ndarray, XM, ref_fit: np.ndarray, what, same: bool):
    """What holds whichever top eigenvector was chosen: proper rotations; aligned = R x + t; the un-refitted rmsd of the aligned fit atoms to the reference
    is the optimum (rmsd_cases' reference and bound); with msel = sel the two sums of squares agree and the mean's fit atoms are centred on c_T."""
    F, n = X.shape[:2]
    fc.check_rotations(got["transforms"], what)
    R, t = got["transforms"][:, :9].reshape(F, 3, 3), got["transforms"][:, 9:]
    measured = X if XM is None else XM
    again = np.einsum("fab,fib->fia", R, measured) + t[:, None]
    size = max(np.abs(measured).max(), np.abs(t).max())
    assert np.abs(again - got["aligned"]).max() <= 8.0 * fc.EPS * size, (what, "aligned = R x + t", np.abs(again - got["aligned"]).max(), size)
    if same:
        best = rc.reference(ref_fit[None], X)
        plain = fc.plain_rmsd(got["aligned"], ref_fit)
        there = max(np.abs(got["aligned"]).max(), np.abs(ref_fit).max())   # (coordinates in the reference's frame: the 4 eps of absolute coordinates)
        assert (np.abs(plain - best["rmsd"][0]) <= best["tol"][0] + 4.0 * fc.EPS * there).all(), (what, "optimal", np.abs(plain - best["rmsd"][0]).max())
        lhs, rhs = n * (got["frame_rmsd"].astype(np.float64) ** 2).sum(), F * (got["rmsf"].astype(np.float64) ** 2).sum()
        assert abs(lhs - rhs) <= 2.0 ** -22 * max(lhs, rhs), (what, lhs, rhs)   # each output is rounded to f32 once (2^-24), squared (2^-23), on either side
        c_t = ref_fit.mean(0)
        assert np.linalg.norm(got["mean"].mean(0) - c_t) <= 8.0 * fc.EPS * there, (what, "centred mean")


@pytest.mark.parametrize("case", fc.shapes(), ids=lambda s: f"F{s[0]}-n{s[1]}-{s[2]}-m{s[3]}")
def test_host_shapes(case):
    c = fc.shape_case(*case)
    X, XM = c["frames"][:, c["sel"]], None if c["msel"] is None else c["frames"][:, c["msel"]]
    got = host_of(X, XM)
    assert got["rmsf"].dtype == np.float32 and got["frame_rmsd"].dtype == np.float32 and got["mean"].shape == (case[3], 3) and got["n_rounds"] == 1
    check_invariants(got, X, XM, X[0], case, same=XM is None)
    if case[1] > 2:
        ratio = fc.assert_within(got, fc.reference(X, XM), case)
        if ratio > WORST["ratio"]:
            WORST.update(ratio=ratio, what=case)
    if case[1] == 1 and XM is None:
        assert (got["rmsf"] == 0).all() and (got["frame_rmsd"] == 0).all()


@pytest.mark.parametrize("name", sorted(rc.degenerate_cases()))
def test_host_degenerate(name):
    X = rc.degenerate_cases()[name]
    got = host_of(X)
    check_invariants(got, X, None, X[0], name, same=True)
    if name in fc.THROUGH_R:
        ref = fc.reference(X)
        ratio = fc.assert_within(got, ref, name)
        if ratio > WORST["ratio"]:
            WORST.update(ratio=ratio, what=name)
        if name in ("tumble", "drift"):
            fc.assert_rigid(got, ref, X[0], name)
    if name == "mirror":
        assert got["frame_rmsd"][1] > 1.0 and fc.plain_rmsd(got["aligned"], X[0])[1] > 1.0


def test_host_external_reference_and_other_frames():
    c = fc.shape_case(33, 64, "disjoint", 65)
    X, XM = c["frames"][:, c["sel"]], c["frames"][:, c["msel"]]
    for ref in (5, 32):
        fc.assert_within(host_of(X, XM, ref=ref), fc.reference(X, XM, ref=ref), ("frame", ref))
    other = X[7] + np.random.default_rng(1).normal(scale=0.5, size=X[7].shape) + 40.0
    got = host_of(X, XM, ref=other)
    fc.assert_within(got, fc.reference(X, XM, ref=other), "external")
    assert np.linalg.norm(got["mean"].mean(0) - other.mean(0)) < 50.0   # the measured mean sits in the reference's frame


@pytest.mark.parametrize("name", sorted(fc.ITERATED))
def test_host_iterated(name):
    fx = fc.iterated_fixture(name)
    X = fx["frames"]
    got = host_of(X, max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"])
    ref = fc.reference(X, max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"])
    assert got["n_rounds"] == ref["n_rounds"] == fx["rounds"] and got["last_change"] <= fx["tol"]
    ratio = fc.assert_within(got, ref, name)
    WORST["iterated"] = max(WORST["iterated"], ratio)
    back = host_of(X, ref=fx["frames"].shape[0] - 1, max_rounds=fc.ITERATED_ROUNDS, tol=fx["tol"])   # started from the last frame: the same structure, turned
    # Both runs stop within tol / 9 (rms over the atoms) of the iteration's fixed point -- the changes shrink tenfold per round -- so their rmsf differ, as
    # an rms over the atoms, by less than tol, plus the iterated bound of either
    diff = back["rmsf"].astype(np.float64) - got["rmsf"]
    assert np.sqrt((diff ** 2).mean()) <= fx["tol"] + 2.0 * (ref["bound"]["rmsf"] * ref["scale"]).max(), (name, np.sqrt((diff ** 2).mean()))


def test_host_cap():
    got = host_of(fc.cap_case(), max_rounds=fc.ITERATED_ROUNDS, tol=fc.CAP_TOL)
    assert got["n_rounds"] == fc.ITERATED_ROUNDS and got["last_change"] > fc.CAP_TOL
    one = host_of(fc.cap_case(), max_rounds=1, tol=1e9)
    assert one["n_rounds"] == 1


def test_host_worst_ratio_is_reported():
    print(f"largest host error / bound: one round {WORST['ratio']:.4f} at {WORST['what']}; iterated {WORST['iterated']:.4f}")
    assert WORST["ratio"] <= 1.0 and WORST["iterated"] <= 1.0


def test_host_refusals():
    x = np.zeros((2, 3, 3))
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, np.zeros((2, 0, 3)), match="selection is empty")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, np.zeros((0, 3, 3)), match="at least one frame")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, x, np.zeros((2, 0, 3)), match="measured selection is empty")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, x, max_rounds=0, match="max_rounds")
    for tol in (-1.0, float("nan"), float("inf")):
        refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, x, tol=tol, match="tol")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, x, reference=2, match="ref_frame 2")
    bad = x.copy()
    bad[1, 2, 0] = np.inf
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, bad, match="frame 1, atom 2")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, x, bad[:, 1:], match="measured coordinate in frame 1, atom 1")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsf_host, x, reference=bad[1], match="ref_sel, atom 2")
    with pytest.raises(ValueError):
        aa.rmsf_host(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        aa.rmsf_host(x, np.zeros((3, 3, 3)))
    with pytest.raises(ValueError):
        aa.rmsf_host(x, reference=np.zeros((4, 3)))


# ---- what arp_rmsf decides before the device is touched ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


def frames_of(s: aa.Structure, F: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)[None].repeat(F, 0)


def raw(s, frames, sel, msel=None, ref=None, ref_frame=0, max_rounds=1, tol=0.0) -> tuple:
    """The ABI call with ctx == NULL: (status, message)."""
    n_frames, ptr, keep = aa.api._frames_arg(s, frames, "rmsf")
    u32 = lambda a: (a if len(a) else np.zeros(1, "<u4")).ctypes.data_as(C.POINTER(C.c_uint32))
    sel = np.ascontiguousarray(sel, "<u4")
    mk = None if msel is None else np.ascontiguousarray(msel, "<u4")
    rk = None if ref is None else np.ascontiguousarray(ref, "<f8")
    st = lib.arp_rmsf(None, s._h, int(n_frames), ptr, u32(sel), len(sel), None if mk is None else u32(mk), 0 if mk is None else len(mk),
                      None if rk is None else rk.ctypes.data_as(C.POINTER(C.c_double)), int(ref_frame), int(max_rounds), C.c_double(tol), *([None] * 7))
    return st, lib.arp_last_error().decode()


def test_null_context_runs_only_the_checks(ubq):
    f = frames_of(ubq, 3)
    assert raw(ubq, f, [0, 5, 9])[0] == _lib.ARP_OK
    assert raw(ubq, None, [0])[0] == _lib.ARP_OK   # the structure's one model is the one frame
    assert raw(ubq, f, [1, 2], msel=[0, 1, 7], ref_frame=2, max_rounds=50, tol=1e-4)[0] == _lib.ARP_OK
    assert raw(ubq, f, [1, 2], ref=f[0], ref_frame=99)[0] == _lib.ARP_OK   # ref_frame is not looked at next to ref_xyz


def test_selection_checks(ubq):
    f = frames_of(ubq, 2)
    N = f.shape[1]
    for sel, words in (([], "selection is empty"), ([0, N], "not an atom of the topology"), ([3, 3], "not strictly increasing"), ([5, 4], "not strictly increasing")):
        st, msg = raw(ubq, f, sel)
        assert st == _lib.ARP_ERR_BAD_INPUT and words in msg and msg.startswith("rmsf: "), (sel, msg)
    for msel, words in (([], "measured selection is empty"), ([0, N], "msel[1]"), ([3, 3], "msel is not strictly increasing"), ([5, 4], "msel is not strictly increasing")):
        st, msg = raw(ubq, f, [0, 1], msel=msel)
        assert st == _lib.ARP_ERR_BAD_INPUT and words in msg and msg.startswith("rmsf: "), (msel, msg)


def test_round_and_reference_checks(ubq):
    f = frames_of(ubq, 3)
    st, msg = raw(ubq, f, [0, 1], max_rounds=0)
    assert st == _lib.ARP_ERR_BAD_INPUT and "max_rounds must be at least 1" in msg
    for tol in (-1e-9, float("nan"), float("inf")):
        st, msg = raw(ubq, f, [0, 1], tol=tol)
        assert st == _lib.ARP_ERR_BAD_INPUT and msg.startswith("rmsf: tol"), (tol, msg)
    st, msg = raw(ubq, f, [0, 1], ref_frame=3)
    assert st == _lib.ARP_ERR_BAD_INPUT and msg.startswith("rmsf: ref_frame 3")
    ref = f[0].copy()
    ref[11, 2] = np.inf
    st, msg = raw(ubq, f, [0, 1], ref=ref)
    assert st == _lib.ARP_ERR_BAD_INPUT and "non-finite coordinate in ref_xyz, atom 11" in msg


def test_frame_checks_are_those_of_the_frequency_call(ubq):
    def freq(frames):
        n_frames, ptr, keep = aa.api._frames_arg(ubq, frames, "contact frequencies")
        t = C.c_void_p()
        return lib.arp_contact_frequencies(None, ubq._h, int(n_frames), ptr, b"/", 0.1, 6.5, C.byref(t)), lib.arp_last_error().decode()

    bad = frames_of(ubq, 3)
    bad[2, 17, 1] = np.nan
    for frames, words in ((frames_of(ubq, 0), "at least one frame"), (bad, "frame 2, atom 17")):
        want = freq(frames)
        assert want[0] == _lib.ARP_ERR_BAD_INPUT and words in want[1]
        assert raw(ubq, frames, [], msel=[], ref_frame=99, max_rounds=0, tol=-1.0) == want   # they come before the call's own checks


def test_input_errors_come_before_the_missing_device(ubq):
    """Whatever the machine: a bad input is ARP_ERR_BAD_INPUT (or a ValueError of the Python layer) from every layer, never ARP_ERR_NO_DEVICE."""
    f = frames_of(ubq, 2)
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsf, ubq, f, fit="ca", chains="Z", match="selection is empty")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsf, ubq, f, atoms=np.zeros(0, np.int64), match="measured selection is empty")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsf, ubq, f, max_rounds=0, match="max_rounds")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsf, ubq, f, tol=-1.0, match="tol")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsf, ubq, f, reference=2, match="ref_frame 2")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsf, ubq, f, reference=np.zeros((4, 3)), match="shape")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsf, ubq, np.zeros((2, 5, 3)), match="shape")
    for kw in (dict(reference="median"), dict(reference=-1), dict(level="chain"), dict(fit="sidechain"), dict(max_rounds=-2)):
        with pytest.raises(ValueError):
            aa.get_rmsf(ubq, f, **kw)


# ---- residues ------------------------------------------------------------------------------------------------------------------------------------------------
def test_residue_rows_by_hand():
    chain = [b"B", b"A", b"A", b"A", b"B", b"A"]
    resi = [1, 2, 2, 1, 1, 2]
    ins = [b"", b"", b"", b"", b"", b"A"]
    r = np.array([3.0, 1.0, 7.0, 2.0, 4.0, 6.0], np.float32)
    got = aa.rmsf_residues(chain, resi, ins, r)
    # rows in (chain, resi, insertion) order: A 1 (atom 3), A 2 (atoms 1, 2), A 2A (atom 5), B 1 (atoms 0, 4)
    assert got["first"].tolist() == [3, 1, 5, 0] and got["n_atoms"].tolist() == [1, 2, 1, 2]
    want = np.array([2.0, np.sqrt((1.0 + 49.0) / 2.0), 6.0, np.sqrt((9.0 + 16.0) / 2.0)])
    assert got["rmsf"].dtype == np.float32 and np.array_equal(got["rmsf"], want.astype(np.float32))
    assert got["bfactor"].dtype == np.float32 and np.allclose(got["bfactor"], 8.0 * np.pi ** 2 / 3.0 * want ** 2, rtol=2.0 ** -22)
    rows, value = fc.residue_rmsf(list(zip(chain, resi, ins)), r)
    assert np.array_equal(value.astype(np.float32), got["rmsf"]) and len(rows) == 4
    empty = aa.rmsf_residues([], [], [], np.zeros(0, np.float32))
    assert len(empty["rmsf"]) == 0 and len(empty["first"]) == 0


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------------------
def test_cli_defaults_and_flags(tmp_path):
    from arpeggia_amd.__main__ import build_parser

    p = build_parser()
    a = p.parse_args(["rmsf", "-i", "x.pdb", "-o", str(tmp_path)])
    assert a.fit == "ca" and a.atoms is None and a.chains == "" and a.reference == "mean" and a.max_rounds == 50 and a.tol == 1e-4 and a.level == "atom"
    assert a.frames is None and a.aligned is None and a.filename == "rmsf"
    a = p.parse_args(["rmsf", "-i", "x.pdb", "-o", str(tmp_path), "--fit", "backbone", "--atoms", "heavy", "-c", "A,B", "--reference", "3", "--max-rounds", "7", "--tol", "0.01",
                      "-l", "residue", "--frames", "f.csv", "--aligned", "a.npy"])
    assert a.fit == "backbone" and a.atoms == "heavy" and a.chains == "A,B" and a.reference == 3 and a.max_rounds == 7 and a.tol == 0.01 and a.level == "residue"
    assert str(a.frames) == "f.csv" and str(a.aligned) == "a.npy"
    for argv in (["rmsf", "-i", "x.pdb"], ["rmsf", "-i", "x.pdb", "-o", str(tmp_path), "--fit", "sidechain"], ["rmsf", "-i", "x.pdb", "-o", str(tmp_path), "--reference", "median"],
                 ["rmsf", "-i", "x.pdb", "-o", str(tmp_path), "--reference", "-1"], ["rmsf", "-i", "x.pdb", "-o", str(tmp_path), "-l", "chain"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
