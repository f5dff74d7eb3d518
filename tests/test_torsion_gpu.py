"""Torsion angles (arp_torsions) on the device.

k_torsion_angle / k_torsion_slab / the histogram kernels / k_torsion_sums / k_torsion_stats against the host twin arp_torsions_host on cases of
tests/torsion_cases.py (each keeps every angle 10^-6 degrees from the bin edges it is run with, so the two must agree exactly except for the last bits of the
f32 angles and the order of the sums): the two files, jittered frames, D around a wave, F around a slab, repeated and overlapping quads, undefined torsions;
identical bytes from call to call and from pass size to pass size, with the only transition on a pass or slab boundary; both routes of the Ramachandran
maps and the contention case; the identities between the outputs; rigid motion; the models of a structure as frames; errors; the command line.  Expected
values never come from the call under test, except where bit-equality between two calls is the property.

The decision edges (exact angles on bin edges, subnormal sines, c = -0.5 one ulp at a time), more than one chunk of k_torsion_stats and the partial waves of
k_torsion_hist2_match are in tests/test_torsion_edge_gpu.py (cases: tests/torsion_edge_cases.py).
"""
from __future__ import annotations

import csv
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import arpeggia_amd as aa
import dssp_cases as dc
import torsion_cases as tc
import trajectory_shapes as ts
from arpeggia_amd import _lib

pytestmark = pytest.mark.gpu

KNOBS = ("rmsd_chunk_atoms", "torsion_hist2_route", "rmsd_cap_bytes")
EXACT = ("cossin", "states", "n_defined", "state_counts", "n_transitions", "hist", "hist2")
ALL = EXACT + ("angles", "sums")


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


@lru_cache(maxsize=None)
def ubq():
    s = aa.Structure.load(str(tc.DATA / "1ubq.pdb"))
    soa = s.soa()
    return s, aa.torsion_select(s), np.stack([soa["x"], soa["y"], soa["z"]], 1).astype(np.float64)


@lru_cache(maxsize=None)
def bft():
    s = aa.Structure.load(str(tc.DATA / "6bft.pdb"))
    soa = s.soa()
    return s, aa.torsion_select(s), np.stack([soa["x"], soa["y"], soa["z"]], 1).astype(np.float64)


@lru_cache(maxsize=None)
def cases() -> dict:
    """name -> (structure, case, pairs, G): the cases of the device-equals-twin comparison, built once; the margins are asserted where each is built."""
    s, sel, xyz = ubq()
    s6, sel6, xyz6 = bft()
    N = len(xyz)
    out = {"1ubq": (s, tc.case("1ubq", xyz[None], sel["quads"], (36, 72)), sel["pairs"], 4),
           "6bft": (s6, tc.case("6bft", xyz6[None], sel6["quads"], (36, 72)), sel6["pairs"], 4),
           "1ubq_jitter33": (s, tc.jittered("1ubq_jitter33", xyz, sel["quads"], 33, 11, (1, 36, 72, 360)), sel["pairs"], 4)}
    for D in (1, 63, 64, 65, 129):
        out[f"D{D}"] = (s, tc.jittered(f"D{D}", xyz, sel["quads"][:D], 3, 40 + D), None, 0)
    for F in (1, 31, 32, 33, 65):
        out[f"F{F}"] = (s, tc.jittered(f"F{F}", xyz, sel["quads"], F, 100 + F), sel["pairs"], 4)
    # repeated and overlapping quads: every window of four consecutive atoms of the first 100, the first ten windows three times over
    windows = np.arange(100)[:, None] + np.arange(4)[None]
    quads = np.concatenate([windows, windows[:10], windows[:10]])
    out["overlap"] = (s, tc.jittered("overlap", xyz, quads, 5, 7), np.array([[0, 100, 0], [1, 1, 1], [50, 51, 1]], "<u4"), 2)
    # undefined torsions mixed in: quads with a repeated atom in every frame, and N, CA, C of residue 1 on a line of integer points in frames 2 and 5
    frames = ts.jitter(xyz, 7, 5)
    for f in (2, 5):
        frames[f, :3] = tc.COLLINEAR[:3] + 10.0
    line = np.array([[0, 1, 2, 3], [0, 1, 2, 9], [5, 5, 6, 7], [5, 6, 6, 7], [5, 6, 7, 7]])
    quads = np.concatenate([line, sel["quads"]])
    pairs = np.concatenate([np.array([[0, 1, 0], [0, 5, 1], [2, 6, 4]], "<u4"), sel["pairs"] + np.array([5, 5, 0], "<u4")])
    out["undefined"] = (s, tc.case("undefined", frames, quads), pairs, 5)
    assert len(tc.SKIPPED_SEEDS) <= 1
    assert len(xyz) == N
    return out


def call(ctx_h, structure, frames, quads, B, pairs=None, G=0, angles=True, cossin=True, states=True, hist=True) -> dict:
    """arp_torsions on caller-given quads (Context.torsions builds them with torsion_select)."""
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    frames = np.ascontiguousarray(frames, "<f8")
    quads = np.ascontiguousarray(quads, "<u4").reshape(-1, 4)
    pr = np.zeros((1, 3), "<u4") if pairs is None else np.ascontiguousarray(pairs, "<u4").reshape(-1, 3)
    P = 0 if pairs is None or not G else len(pr)
    F, D = len(frames), len(quads)
    out = aa.api._torsion_outputs(F, D, B if hist else 0, G if P else 0, angles, cossin, states)
    st = _lib.lib.arp_torsions(ctx_h, structure._h, F, frames.ctypes.data_as(dp), quads.ctypes.data_as(u32p), D, B, pr.ctypes.data_as(u32p), P, G if P else 0,
                               *aa.api._torsion_pointers(out))
    if st != _lib.ARP_OK:
        raise aa.ArpeggiaError(st, _lib.lib.arp_last_error().decode())
    return out


def device(ctx, name: str, B: int = 36, **kw) -> dict:
    s, c, pairs, G = cases()[name]
    return call(ctx._h, s, c["frames"], c["quads"], B, pairs, G, **kw)


@lru_cache(maxsize=None)
def host(name: str, B: int = 36) -> dict:
    """The host twin on a case, computed once."""
    _, c, pairs, G = cases()[name]
    return aa.torsions_host(tc.gather(c["frames"], c["quads"]), pairs, G, B)


def assert_equal(got: dict, want: dict, what):
    for key in EXACT:
        if key in want or key in got:
            assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5].tolist())
    g, w = got["angles"], want["angles"]
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g.view("<u4")[np.isnan(g)], w.view("<u4")[np.isnan(w)]), (what, "NaN pattern")
    ok = ~np.isnan(w)
    ulp = np.spacing(np.maximum(np.abs(g[ok]), np.abs(w[ok])).astype(np.float32))
    assert (np.abs(g[ok].astype(np.float64) - w[ok]) <= 4.0 * ulp).all(), (what, "angles")
    F = g.shape[0]
    bound = F * 2.0 ** -52 * want["n_defined"].astype(np.float64)[:, None]   # both orders err by at most gamma_(F - 1) sum |term|, |term| <= 1
    assert (np.abs(got["sums"] - want["sums"]) <= bound).all(), (what, "sums", float(np.abs(got["sums"] - want["sums"]).max()))


def same_bytes(a: dict, b: dict, what):
    assert set(a) == set(b)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


NAMES = ["1ubq", "6bft", "1ubq_jitter33", "D1", "D63", "D64", "D65", "D129", "F1", "F31", "F32", "F33", "F65", "overlap", "undefined"]


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host(ctx, name):
    assert sorted(NAMES) == sorted(cases())
    got = device(ctx, name)
    assert_equal(got, host(name), name)
    _, c, pairs, G = cases()[name]
    F, D = len(c["frames"]), len(c["quads"])
    assert got["angles"].shape == (F, D) and got["cossin"].shape == (F, D, 2) and got["hist"].shape == (D, 36)
    if name == "undefined":
        assert got["states"][:, 2:5].max() == 0 and got["states"][[2, 5], :2].max() == 0 and got["states"][[0, 1, 3, 4, 6], :2].min() > 0
        assert got["n_defined"][:5].tolist() == [5, 5, 0, 0, 0] and int(got["hist2"][4].sum()) == 0


@pytest.mark.parametrize("B", [1, 72, 360])
def test_bin_counts(ctx, B):
    """hist at 1, 72 and 360 bins (36: every other test); hist2 of the four classes at 72 bins is 83 KB, past the LDS tables: the wave-matched route."""
    assert (4 * 72 * 72 * 4 > tc.LDS_BYTES) and (4 * 36 * 36 * 4 <= tc.LDS_BYTES)
    assert_equal(device(ctx, "1ubq_jitter33", B), host("1ubq_jitter33", B), B)
    if B == 72:
        assert_equal(device(ctx, "6bft", B), host("6bft", B), "6bft 72")


def test_pass_size_and_repeat_give_the_same_bytes(ctx):
    """1ubq x 33 frames in 1, 2 and 33 upload passes, and twice in a row: every output byte for byte (a slab of 32 frames is cut by every pass boundary but one)."""
    s, c, _, _ = cases()["1ubq_jitter33"]
    N = c["frames"].shape[1]
    first = device(ctx, "1ubq_jitter33")
    same_bytes(device(ctx, "1ubq_jitter33"), first, "repeat")
    for per, passes in ((17, 2), (1, 33)):
        assert -(-33 // per) == passes
        aa.debug_set("rmsd_chunk_atoms", per * N)
        same_bytes(device(ctx, "1ubq_jitter33"), first, passes)
    assert first["n_transitions"].sum() > 0


@pytest.mark.parametrize("F,at,pers", [(6, 3, (6, 3, 1)), (40, 32, (40, 20, 1)), (40, 32, (32, 8))])
def test_the_only_transition_on_a_boundary(ctx, F, at, pers):
    """One built torsion, g+ in the frames before `at` and t from it on: the only transition lies between frames at - 1 and at -- exactly on a pass boundary
    (6 frames in passes of 3; 40 frames in passes of 32 or 8), exactly on the slab boundary 31 | 32, or inside a pass: one transition, the same bytes."""
    quad = tc.state_frames([1] * at + [2] * (F - at))
    s = aa.Structure.from_records(ts.records(tc.four_atoms(quad[0])))
    first = None
    for per in pers:
        aa.debug_set("rmsd_chunk_atoms", per * 4)
        got = call(ctx._h, s, quad, [[0, 1, 2, 3]], 36)
        assert got["n_transitions"].tolist() == [1] and got["state_counts"].tolist() == [[0, at, F - at, 0]]
        first = first or got
        same_bytes(got, first, per)
    assert_equal(first, aa.torsions_host(quad[:, None]), (F, at))


def test_both_routes_of_the_maps(ctx):
    """The class groups (4 x 36 x 36 words: LDS tables) and one group per residue (76 x 36 x 36: wave-matched global adds), each against the twin; and the three
    routes forced on the class groups: the same bytes."""
    s, sel, _ = ubq()
    _, c, pairs, _ = cases()["1ubq_jitter33"]
    want = host("1ubq_jitter33")
    auto = device(ctx, "1ubq_jitter33")
    assert np.array_equal(auto["hist2"], want["hist2"])
    for route in (1, 2, 3):
        aa.debug_set("torsion_hist2_route", route)
        same_bytes(device(ctx, "1ubq_jitter33"), auto, route)
    aa.debug_set("torsion_hist2_route", 0)
    R = sel["n_rows"]
    assert R * 36 * 36 * 4 > tc.LDS_BYTES
    per_res = pairs.copy()
    per_res[:, 2] = sel["row"][pairs[:, 0]]
    got = call(ctx._h, s, c["frames"], c["quads"], 36, per_res, R)
    twin = aa.torsions_host(tc.gather(c["frames"], c["quads"]), per_res, R, 36)
    assert np.array_equal(got["hist2"], twin["hist2"]) and got["hist2"].shape == (R, 36, 36)
    assert np.array_equal(got["hist2"].sum((1, 2)), np.bincount(per_res[:, 2], minlength=R) * 33)
    through = ctx.torsions(s, c["frames"], rama="residue")
    assert np.array_equal(through["hist2"], got["hist2"]) and through["n_groups"] == R
    assert np.array_equal(ctx.torsions(s, c["frames"])["hist2"], auto["hist2"])


@pytest.mark.parametrize("route", [0, 2])
def test_contention_case(ctx, route):
    """1000 identical frames of a built alpha helix, one group: every sample of a pair lands in that pair's one bin, which holds exactly F per pair that shares
    it, and the table sums to F P.  The expected bins come from the restatement on one frame."""
    F = 1000
    helix = dc.helix("alpha")
    s = aa.Structure.from_records(dc.records(helix))
    sel = aa.torsion_select(s, kinds=("phi", "psi"))
    P = len(sel["pairs"])
    assert P == dc.HELIX_RESIDUES - 2
    one = dc.frames_of(helix)
    assert tc.clear(one, sel["quads"], (36,))
    bins = tc.restate(tc.gather(one, sel["quads"]), 36)["bin"][0]
    want = np.zeros((1, 36, 36), np.uint32)
    for a, b, _ in sel["pairs"]:
        want[0, bins[a], bins[b]] += F
    pairs = sel["pairs"].copy()
    pairs[:, 2] = 0
    aa.debug_set("torsion_hist2_route", route)
    got = call(ctx._h, s, np.repeat(one, F, 0), sel["quads"], 36, pairs, 1, angles=False, cossin=False, states=False)
    assert np.array_equal(got["hist2"], want) and int(got["hist2"].sum()) == F * P
    assert (got["hist"].max(1) == F).all() and (got["n_transitions"] == 0).all() and (got["n_defined"] == F).all()


def test_identities_between_the_outputs(ctx):
    s, c, pairs, G = cases()["undefined"]
    F, D = len(c["frames"]), len(c["quads"])
    full = device(ctx, "undefined", states=True)
    st = full["states"]
    assert np.array_equal(full["state_counts"][:, 1:].sum(1), full["n_defined"]) and (full["state_counts"].sum(1) == F).all()
    assert np.array_equal(full["hist"].sum(1), full["n_defined"])
    assert int(full["hist2"].sum()) == int(((st[:, pairs[:, 0]] != 0) & (st[:, pairs[:, 1]] != 0)).sum())
    assert np.array_equal(full["n_defined"], (st != 0).sum(0)) and np.array_equal(full["n_defined"], (~np.isnan(full["angles"])).sum(0))
    assert (full["cossin"][st == 0] == 0).all() and np.abs(np.hypot(full["cossin"][..., 0], full["cossin"][..., 1])[st != 0] - 1.0).max() <= 4 * 2.0 ** -53
    bare = call(ctx._h, s, c["frames"], c["quads"], 0, None, 0, angles=False, cossin=False, states=False, hist=False)
    assert set(bare) == {"sums", "n_defined", "state_counts", "n_transitions"}
    for key in bare:
        assert bare[key].tobytes() == full[key].tobytes(), key
    only_hist = call(ctx._h, s, c["frames"], c["quads"], 36, None, 0, angles=False, cossin=False, states=False)
    assert "hist2" not in only_hist and only_hist["hist"].tobytes() == full["hist"].tobytes()


def test_through_python_and_the_statistics(ctx):
    s, sel, _ = ubq()
    _, c, _, _ = cases()["1ubq_jitter33"]
    res = ctx.torsions(s, c["frames"], cossin=True, states=True)
    want = host("1ubq_jitter33")
    assert_equal(res, want, "python")
    for key in ("quads", "kind", "residue", "row", "rama_class"):
        assert np.array_equal(res[key], sel[key])
    # the statistics from the restatement: circular mean, resultant, circular standard deviation
    r = tc.restate(tc.gather(c["frames"], c["quads"]))
    C_, S_ = r["c"].sum(0), r["s"].sum(0)
    assert np.abs(res["mean"] - np.degrees(np.arctan2(S_, C_))).max() <= 1e-9
    assert np.abs(res["resultant"] - np.hypot(C_, S_) / 33).max() <= 1e-13
    assert np.abs(res["circ_std"] - np.degrees(np.sqrt(-2 * np.log(np.hypot(C_, S_) / 33)))).max() <= 1e-6
    assert res["state_fraction"].dtype == np.float32 and np.array_equal(res["state_fraction"], (want["state_counts"][:, 1:] / 33).astype("<f4"))
    lean = ctx.torsions(s, c["frames"], kinds=("chi",), bins=0, rama=None, angles=False)
    assert "angles" not in lean and "hist" not in lean and "hist2" not in lean and set(lean["kind"].tolist()) == {3, 4, 5, 6, 7}


def test_models_are_the_frames(ctx):
    helix = dc.jittered(dc.device_cases()["helix_alpha"], 5, 3)
    models = aa.Structure.from_records(dc.model_records(helix))
    one = aa.Structure.from_records(dc.records(helix))
    got, want = ctx.torsions(models, None, cossin=True, states=True), ctx.torsions(one, dc.frames_of(helix), cossin=True, states=True)
    for key in ALL:
        assert got[key].tobytes() == want[key].tobytes(), key
    assert got["angles"].shape == (5, 3 * dc.HELIX_RESIDUES - 3)


def test_rigid_motion_keeps_the_states(ctx):
    """A tumble, and a shift of 10^4 A.  The shifted coordinates are rounded to the spacing of f64 at 10^4, 2^-39: each lies within e = 2^-40 of the shifted point
    (the unshifted file coordinates are exact).  Moving atom k by |delta| turns a torsion by at most |delta| / (r sin t) for an end atom and 2.2 |delta| / (r sin t)
    for a middle atom (r the bond length >= 1.2 A, t the bond angle with sin t >= 0.7, |b.b'| / |b'|^2 <= 0.6): in all at most 6.4 sqrt(3) e / 0.84 = 1.2e-11 rad,
    so c and s move by no more than that plus their own rounding."""
    s, sel, xyz = ubq()
    base = call(ctx._h, s, xyz[None], sel["quads"], 36, sel["pairs"], 4)
    frames = ts.tumble(xyz, 5, 4)
    assert tc.clear(frames, sel["quads"], (36,))
    got = call(ctx._h, s, frames, sel["quads"], 36, sel["pairs"], 4)
    assert (got["states"] == base["states"][0]).all() and (got["n_transitions"] == 0).all() and (got["hist"] == 5 * base["hist"]).all()
    assert np.array_equal(got["hist2"], 5 * base["hist2"])
    shifted = xyz[None] + 1.0e4 * ts.DRIFT_DIRECTION
    far = call(ctx._h, s, shifted, sel["quads"], 36, sel["pairs"], 4)
    assert np.array_equal(far["states"], base["states"])
    tol = 6.4 * np.sqrt(3.0) * 2.0 ** -40 / (1.2 * 0.7) + 2.0 ** -52
    assert np.abs(far["cossin"] - base["cossin"]).max() <= tol, float(np.abs(far["cossin"] - base["cossin"]).max())
    assert np.abs(far["angles"].astype(np.float64) - base["angles"]).max() <= np.degrees(tol) + 2.0 ** -16      # (and one f32 spacing at 180)


def test_files_end_to_end_and_the_command_line(ctx, tmp_path):
    from arpeggia_amd.__main__ import main

    res = aa.torsions(str(tc.DATA / "1ubq.pdb"))
    want = host("1ubq")
    for key in ("n_defined", "state_counts", "n_transitions", "hist", "hist2"):
        assert np.array_equal(res[key], want[key]), key
    assert (np.abs(res["angles"].astype(np.float64) - want["angles"]) <= 4.0 * np.spacing(np.abs(want["angles"]))).all() and "cossin" not in res and "states" not in res
    heavy = aa.get_torsions(aa.Structure.load(str(tc.DATA / "6bft.pdb")), chains="H,L", kinds="phi,psi", angles=False)
    assert "angles" not in heavy and heavy["hist2"].shape == (4, 36, 36) and int(heavy["hist2"].sum()) == len(heavy["pairs"])
    out = tmp_path / "out"
    assert main(["torsions", "-i", str(tc.DATA / "1ubq.pdb"), "-o", str(out), "--angles", str(tmp_path / "angles.npy"), "--rama-file", str(tmp_path / "rama.npy")]) == 0
    with open(out / "torsions.csv", newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == aa.TORSION_COLUMNS and len(lines) == 387
    assert [row[4] for row in lines[1:8]] == ["psi", "omega", "chi1", "chi2", "chi3", "phi", "psi"] and [row[2] for row in lines[1:8]] == ["1"] * 5 + ["2"] * 2
    assert abs(float(lines[1][6]) - 149.6288) <= 1e-3 and lines[1][5] == "1" and lines[1][12] == "0"
    assert [float(v) for v in lines[3][9:12]] == [1.0, 0.0, 0.0]       # chi1 of MET 1 = 80.4: g+
    assert np.load(tmp_path / "angles.npy").tobytes() == res["angles"].tobytes()
    assert np.load(tmp_path / "rama.npy").tobytes() == res["hist2"].tobytes()
    assert main(["torsions", "-i", str(tc.DATA / "1ubq.pdb"), "--rama", "residue", "--bins", "72", "--rama-file", str(tmp_path / "r2.npy")]) == 0
    assert np.load(tmp_path / "r2.npy").shape == (76, 72, 72)
    assert main(["torsions", "-i", str(tc.DATA / "1ubq.pdb")]) == 1    # nothing to write
    assert main(["torsions", "-i", str(tc.DATA / "1ubq.pdb"), "--kinds", "omega", "--rama-file", str(tmp_path / "none.npy")]) == 1    # no pair, no map


def test_errors_through_python(ctx):
    s, sel, xyz = ubq()
    frames = np.repeat(xyz[None], 2, 0)
    with pytest.raises(aa.ArpeggiaError, match=rf"torsions: frames must have shape \[F, {len(xyz)}, 3\]"):
        ctx.torsions(s, frames[:, :40])
    frames[1, 9, 2] = np.inf
    with pytest.raises(aa.ArpeggiaError, match="non-finite coordinate in frame 1, atom 9"):
        ctx.torsions(s, frames)
    with pytest.raises(aa.ArpeggiaError, match="at least one frame is needed"):
        ctx.torsions(s, frames[:0])
    with pytest.raises(aa.ArpeggiaError, match=r"torsions: no torsions \(n_tors == 0\)"):
        ctx.torsions(s, None, chains="Z")
    with pytest.raises(aa.ArpeggiaError, match="torsions: n_bins = 400"):
        ctx.torsions(s, None, bins=400)
    aa.debug_set("rmsd_cap_bytes", 1000)
    with pytest.raises(aa.ArpeggiaError, match="rmsd_cap_bytes") as e:
        ctx.torsions(s, None)
    assert e.value.status == _lib.ARP_ERR_CAPACITY
