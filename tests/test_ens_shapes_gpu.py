"""The ensemble paths on frames that drift, tumble, swell, collapse and go flat, on the MI355X.

Every ensemble test before this one built its frames as base + 0.3 A jitter: all frames of a pass shared one box to within an angstrom, so the
per-frame origin and midpoint, the grid sized over all frames, the separator layer between the slabs and the coarsening loop of the packed grid
(grid.inl: k_model_bounds, setup_block, grid_setup, cell_index, place_atom) were never asked anything.  tests/trajectory_shapes.py builds frames
that do ask; tests/test_trajectory_shapes_host.py shows on the CPU that every case reaches its mechanism.

Expected values never come from the packed path:
  (a) the per-frame loop over the single-structure device calls that the existing ensemble tests use (ens_sasa_common.frame_loop and
      bsa_frame_loop, expected() and device_reference() of freq_common.py, atom_values() of residue_sasa_common.py), and
  (b) because (a) shares grid.inl with the pack, the CPU restatements on the extreme frames of every case -- the farthest, the swollen, the
      collapsed, the flat ones: sasa_restatement.atom_counts, bsa_common.split_counts, and a plain numpy f64 neighbour sum for SAP.
Counts, SASA / dSASA aggregates, totals and frequency tables are compared for equality; SAP per-frame values within the project's
ens_sasa_common.SAP_TOL of the loop, SAP aggregates exactly from the path's own per-frame values.  No tolerance is new.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import bsa_common as bc
import ens_sasa_common as ec
import freq_ring_cases as frc
import residue_sasa_common as rc
import sasa_restatement as sr
import trajectory_shapes as ts
from ens_sasa_common import SASA_KEYS, assert_sap_aggregates, assert_sap_close, assert_sasa_equal, bits, bsa_frame_loop
from freq_common import assert_same_rows, assert_table_equal, atom_part, device_reference, ring_part, to_bytes
from freq_common import expected as freq_expected
from residue_sasa_common import atom_values, expected_levels

pytestmark = pytest.mark.gpu

F = 16
PROBE, N_POINTS, SAP_RADIUS = 1.4, 100, 10.0
DENSE = ("collapsed", "point", "flat_even", "flat_odd")  # extreme frames whose full restatement is tens of millions of tests: a sample of homes instead
RES_KEYS = ("mean_sasa", "std_sasa", "min_sasa", "max_sasa", "mean_relative_sasa", "chain_sasa", "residue_sasa", "is_polar", "relative_valid", "res_atoms",
            "chain_atoms")
BSA_KEYS = ("buried", "total_complex", "total_g1", "total_g2", "dsasa", "sum_buried", "sum_buried_sq", "min_buried", "max_buried", "frames_buried")


@pytest.fixture(scope="module")
def ctx():
    """The context of the 1ubq x 16 cases and of nothing larger: a context keeps the largest workspace it ever needed, and the swell cases must meet the
    cell capacity tests/test_trajectory_shapes_host.py works with (that of 16 x 660 packed atoms)."""
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


@pytest.fixture(scope="module")
def big_ctx():
    """6bft, the ring topologies and the 65 541-frame cases."""
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    aa.debug_set("ens_chunk_atoms", 0)
    aa.debug_set("freq_chunk_atoms", 0)


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


@pytest.fixture(scope="module")
def bft(bft_path):
    return aa.load_model(bft_path)


@pytest.fixture(scope="module")
def sphere():
    pts = aa.sasa_sphere_points(N_POINTS)
    assert np.array_equal(pts, sr.sphere_points(N_POINTS))
    return pts


_frames = {}


def case_frames(which: str, s, name: str, n_frames: int = F):
    """(frames, extremes) of a named shape on a structure's topology; built once."""
    key = (which, name, n_frames)
    if key not in _frames:
        _frames[key] = ts.make(name, ec.topology_xyz(s), n_frames)
    return _frames[key]


def homes_of(label: str, m: int) -> np.ndarray:
    return np.arange(0, m, 10 if label in DENSE or m > 1000 else 1)


def xyz_of(frame, sel):
    return tuple(np.ascontiguousarray(frame[sel, k]) for k in range(3))


def sap_reference(frame, sel, side, weight, radius: float) -> np.ndarray:
    """The neighbour sum written out in numpy f64: for every side-chain atom the sum of the weights of the side-chain atoms within `radius`
    (inclusive, itself included; the squared radius formed in f32 as sap.rs does), on the untouched f64 coordinates."""
    c = np.asarray(frame, np.float64)[sel][side]
    w = np.asarray(weight, np.float32)[side].astype(np.float64)
    r2 = float(np.float32(radius) * np.float32(radius))
    d = c[:, None, :] - c[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    out = np.zeros(len(sel), np.float64)
    out[side] = ((d2 <= r2) * w[None, :]).sum(1)
    return out


def forced(name: str, n_frames: int = F) -> list:
    return ts.forced_passes(name, n_frames)


# ---- 1. SASA and SAP ------------------------------------------------------------------------------------------------------------------------------
def check_sasa(ctx, which, s, name, chains, sphere, n_frames=F):
    frames, extremes = case_frames(which, s, name, n_frames)
    got = ctx.sasa_ensemble(s, frames, chains, PROBE, N_POINTS, sap_radius=SAP_RADIUS, per_frame=True)
    sel = got["atoms"].astype(np.int64)
    m = len(sel)
    assert got["n_frames"] == n_frames and m > 500
    # (a) the per-frame loop
    want = ec.frame_loop(ctx, s, sel, frames, PROBE, N_POINTS, sap_radius=SAP_RADIUS)
    assert_sasa_equal(got, want, want["R"], N_POINTS)
    assert_sap_close(got["sap"], want["sap"], want["side"])
    assert_sap_aggregates(got)
    # (b) the restatements on the extreme frames
    resn = [v.decode() for v in s.strings("resn")[sel]]
    for label, f in extremes.items():
        homes = homes_of(label, m)
        x, y, z = xyz_of(frames[f], sel)
        counts = sr.atom_counts(x, y, z, want["R"], sphere, homes=homes)
        assert np.array_equal(got["count"][f][homes], counts), (label, f)
        # the weights from the loop's areas (equal to the pack's, and to the restatement's at the homes: asserted above), the sum in numpy
        w = np.array([aa.sap_weight(resn[k], float(want["sasa"][f][k])) for k in range(m)], np.float32)
        ref = sap_reference(frames[f], sel, want["side"], w, SAP_RADIUS)
        tol = ec.SAP_TOL * max(1.0, float(np.abs(ref).max(initial=0.0)))
        assert float(np.abs(got["sap"][f].astype(np.float64) - ref).max(initial=0.0)) <= tol, (label, f)
    # forced passes: the grid differs from pass to pass, the integers do not
    for per in forced(name, n_frames):
        aa.debug_set("ens_chunk_atoms", per * m)
        again = ctx.sasa_ensemble(s, frames, chains, PROBE, N_POINTS, sap_radius=SAP_RADIUS, per_frame=True)
        for k in SASA_KEYS + ("count", "total_sasa", "atoms"):
            assert again[k].tobytes() == got[k].tobytes(), (per, k)
        assert_sap_close(again["sap"], want["sap"], want["side"])
        assert_sap_aggregates(again)
        twice = ctx.sasa_ensemble(s, frames, chains, PROBE, N_POINTS, sap_radius=SAP_RADIUS, per_frame=True)
        assert ec.result_bytes(twice) == ec.result_bytes(again), per
    aa.debug_set("ens_chunk_atoms", 0)
    assert ec.result_bytes(ctx.sasa_ensemble(s, frames, chains, PROBE, N_POINTS, sap_radius=SAP_RADIUS, per_frame=True)) == ec.result_bytes(got)
    return got, want, extremes


@pytest.mark.parametrize("name", ts.SHAPES)
def test_sasa_and_sap_on_1ubq(ctx, ubq, sphere, name):
    got, want, extremes = check_sasa(ctx, "ubq", ubq, name, "", sphere)
    if "swollen" in extremes:  # every atom of the swollen frame is alone
        assert (got["count"][extremes["swollen"]] == N_POINTS).all()
    if "point" in extremes:  # on one point only the largest spheres keep open points
        row, R = got["count"][extremes["point"]], want["R"]
        assert (row[R < R.max()] == 0).all() and (row[R == R.max()] > 0).all()
    if name == "drift":  # the far frame is the near frame on a coarser f32 lattice: close, not equal
        assert 0 < (got["count"][extremes["far"]] != got["count"][extremes["home"]]).sum() < got["count"].shape[1]


def test_sasa_and_sap_on_tumbling_6bft(big_ctx, bft, sphere):
    check_sasa(big_ctx, "bft", bft, "tumble", "H,L", sphere, 8)


# ---- 2. the residue level -------------------------------------------------------------------------------------------------------------------------
def check_residues(ctx, which, s, name, chains, sphere, n_frames=F):
    frames, extremes = case_frames(which, s, name, n_frames)
    got = ctx.residue_sasa_ensemble(s, frames, chains, PROBE, N_POINTS, "protor", per_frame=True)
    sel = rc.select_1_to_4(s, chains).astype(np.int64)
    res, chn = rc.residue_groups(s, sel), rc.chain_groups(s, sel)
    assert got["n_frames"] == n_frames and got["residue_sasa"].shape == (n_frames, len(res)) and got["chain_sasa"].shape == (n_frames, len(chn))
    for f in range(n_frames):  # (a)
        _, res_sum, _, chn_sum = expected_levels(s, sel, atom_values(ctx, s, sel, "protor", N_POINTS, frames[f]))
        assert np.array_equal(bits(got["residue_sasa"][f]), bits(res_sum)), f
        assert np.array_equal(bits(got["chain_sasa"][f]), bits(chn_sum)), f
    r, fell_back = rc.table_radii(s, sel, "protor")
    R = (r + np.float32(PROBE)).astype(np.float32)
    for label, f in extremes.items():  # (b): a residue sum needs every atom of the residue -- the residues of a sample of homes
        keep = [k for k in range(len(res)) if k % (10 if label in DENSE or len(sel) > 1000 else 1) == 0]
        homes = np.array(sorted(a for k in keep for a in res[k][1]), np.int64)
        x, y, z = xyz_of(frames[f], sel)
        values = np.zeros(len(sel), np.float32)
        values[homes] = sr.sasa_from_counts(R[homes], sr.atom_counts(x, y, z, R, sphere, homes=homes), N_POINTS)
        want = np.array([rc.seq_sum(values[res[k][1]]) for k in keep], np.float32)
        assert np.array_equal(bits(got["residue_sasa"][f][keep]), bits(want)), (label, f)
    w = ec.sap_stats(got["residue_sasa"])  # the aggregates from the per-frame values in frame order, as tests/test_residue_sasa_gpu.py restates them
    for k, key in (("mean_sasa", "mean_sap"), ("std_sasa", "std_sap"), ("min_sasa", "min_sap"), ("max_sasa", "max_sap")):
        assert np.array_equal(bits(got[k]), bits(w[key])), k
    want_bytes = b"".join(np.ascontiguousarray(got[k]).tobytes() for k in RES_KEYS)
    for per in forced(name, n_frames) + [0]:
        aa.debug_set("ens_chunk_atoms", per * len(sel))
        again = ctx.residue_sasa_ensemble(s, frames, chains, PROBE, N_POINTS, "protor", per_frame=True)
        assert b"".join(np.ascontiguousarray(again[k]).tobytes() for k in RES_KEYS) == want_bytes, per
    return got


@pytest.mark.parametrize("name", ts.SHAPES)
def test_residue_level_on_1ubq(ctx, ubq, sphere, name):
    got = check_residues(ctx, "ubq", ubq, name, "", sphere)
    assert got["residue_sasa"].shape == (F, 76)


def test_residue_level_on_tumbling_6bft(big_ctx, bft, sphere):
    check_residues(big_ctx, "bft", bft, "tumble", "H,L", sphere, 8)


# ---- 3. dSASA -----------------------------------------------------------------------------------------------------------------------------------
def check_dsasa(ctx, which, s, name, groups, sphere, n_frames=F):
    frames, extremes = case_frames(which, s, name, n_frames)
    got = ctx.dsasa_ensemble(s, frames, groups, PROBE, N_POINTS, per_frame=True)
    sel, mask = got["atoms"].astype(np.int64), got["group"]
    m = len(sel)
    assert got["n_frames"] == n_frames and got["buried"].shape == (n_frames, m) and m > 500
    loop = bsa_frame_loop(ctx, s, got, frames, PROBE, N_POINTS)  # (a)
    assert np.array_equal(got["buried"], loop["buried"])
    for k in ("total_complex", "total_g1", "total_g2", "dsasa"):
        assert np.array_equal(bits(got[k]), bits(loop[k])), k
    b = loop["buried"].astype(np.int64)
    assert np.array_equal(got["sum_buried"], b.sum(0).astype(np.uint64)) and np.array_equal(got["sum_buried_sq"], (b * b).sum(0).astype(np.uint64))
    assert np.array_equal(got["min_buried"], b.min(0)) and np.array_equal(got["max_buried"], b.max(0))
    assert np.array_equal(got["frames_buried"], (b > 0).sum(0).astype(np.uint32))
    for label, f in extremes.items():  # (b)
        homes = homes_of(label, m)
        x, y, z = xyz_of(frames[f], sel)
        _, want_buried = bc.split_counts(x, y, z, got["R"], mask, sphere, homes=homes)
        assert np.array_equal(got["buried"][f][homes], want_buried), (label, f)
    want_bytes = b"".join(np.ascontiguousarray(got[k]).tobytes() for k in BSA_KEYS)
    for per in forced(name, n_frames) + [0]:
        aa.debug_set("ens_chunk_atoms", per * m)
        again = ctx.dsasa_ensemble(s, frames, groups, PROBE, N_POINTS, per_frame=True)
        assert b"".join(np.ascontiguousarray(again[k]).tobytes() for k in BSA_KEYS) == want_bytes, per
    # the table's statistics from the integers (bsa_common.buried_stats)
    _, at = aa.get_dsasa_ensemble(s, frames, groups, PROBE, N_POINTS)
    at = at if hasattr(at, "column") and not hasattr(at, "to_arrow") else at.to_arrow()
    want = bc.buried_stats(n_frames, got["R"], N_POINTS, loop["buried"])
    for k in ("buried_mean", "buried_std", "buried_min", "buried_max"):
        assert np.array_equal(bits(np.array(at.column(k).to_pylist(), np.float32)), bits(want[k])), k
    assert at.column("occupancy").to_pylist() == want["occupancy"].tolist()
    return got


@pytest.mark.parametrize("name", ts.SHAPES)
def test_dsasa_on_1ubq(ctx, ubq, sphere, name):
    got = check_dsasa(ctx, "ubq", ubq, name, "/", sphere)
    assert (got["group"] == 3).all() and (got["buried"] > 0).any()


def test_dsasa_on_tumbling_6bft(big_ctx, bft, sphere):
    got = check_dsasa(big_ctx, "bft", bft, "tumble", "C/H,L", sphere, 8)
    assert set(got["group"].tolist()) == {1, 2} and (got["frames_buried"] == 8).any() and (got["frames_buried"] == 0).any()


# ---- 4. contact frequencies -------------------------------------------------------------------------------------------------------------------------
def check_freq(ctx, s, rec, frames, name, ring_reference=True):
    """rings=False against the atomic_contacts loop, rings=True against the single-structure tables; then the forced passes."""
    n = frames.shape[1]
    plain = ctx.contact_frequencies(s, frames, "/")
    assert_table_equal(plain, freq_expected(ctx, s, frames, "/"))
    with_rings = ctx.contact_frequencies(s, frames, "/", rings=True)
    assert to_bytes(atom_part(with_rings)) == to_bytes(plain)
    want_rings = device_reference(ctx, rec, frames, "/") if ring_reference else None
    if ring_reference:
        assert_same_rows(ring_part(with_rings), want_rings)
    for per in forced(name, len(frames)):
        aa.debug_set("freq_chunk_atoms", per * n)
        assert to_bytes(ctx.contact_frequencies(s, frames, "/")) == to_bytes(plain), per
        assert to_bytes(ctx.contact_frequencies(s, frames, "/", rings=True)) == to_bytes(with_rings), per
    aa.debug_set("freq_chunk_atoms", 0)
    return plain, with_rings, want_rings


@pytest.mark.parametrize("name", ts.SHAPES)
def test_contact_frequencies_on_1ubq(ctx, ubq, ubq_path, name):
    import synth

    frames, extremes = case_frames("ubq", ubq, name)
    plain, _, _ = check_freq(ctx, ubq, synth.read_pdb_records(ubq_path), frames, name)
    assert len(plain["n_frames"]) > 500 and plain["n_frames"].max() <= F
    if name in ("drift", "tumble"):  # rigid motion of one conformation: a contact is there in every frame or (f32 distances at 10^5 A aside) in almost every
        assert (plain["n_frames"] == F).sum() > len(plain["n_frames"]) // 2


_ring_cases = {}
WIDE_ON_ONE_SPOT = ("collapse@first", "collapse@mid", "collapse@last", "flat_xyz", "mixed")  # (with all atoms on one POINT no ring has a plane: that frame fits)


def ring_case(which: str):
    if which not in _ring_cases:
        case = frc.small_case() if which == "small" else frc.wide_case()
        base = case.frames[np.arange(F) % case.F]  # the schedule's own frames: the partners move from frame to frame
        _ring_cases[which] = (case, aa.Structure.from_records(case.rec), base)
    return _ring_cases[which]


@pytest.mark.parametrize("name", ts.SHAPES)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_contact_frequencies_on_the_ring_topologies(ctx, big_ctx, which, name):
    case, s, base = ring_case(which)
    frames, extremes = ts.make(name, base, F)
    # The 292 rings of the wide topology on one spot are 47 000 ring rows in one frame; the single-structure table (get_contacts: the reference of
    # the ring rows, not under test here) reserves 19 712 for 292 rings and refuses the frame with an error.  Those frames keep every other check
    # -- the atom rows against the atomic_contacts loop, the atom part of the ring table, the forced passes -- and the small topology, whose
    # 21 rings fit, holds their ring rows to the reference.
    on_one_spot = which == "wide" and name in WIDE_ON_ONE_SPOT
    _, with_rings, want_rings = check_freq(ctx if which == "small" else big_ctx, s, case.rec, frames, name, ring_reference=not on_one_spot)
    if name == "drift":  # a translation keeps every state of the schedule: the ring rows of the untransformed frames (a rotation need not -- the
        # reference's plane fit fixes the sign of a ring's normal by the axes)
        still = device_reference(big_ctx, case.rec, base, "/")
        for c in ("interaction", "from_ring", "to_ring", "from_atom", "to_atom", "n_frames"):
            assert np.array_equal(want_rings[c], still[c]), c
        assert len(still["interaction"]) > 10 and (ring_part(with_rings)["from_ring"] >= 0).all()


# ---- 5. the order of the frames changes nothing ------------------------------------------------------------------------------------------------------
def test_frame_permutation(ctx, ubq, ubq_path):
    frames, _ = case_frames("ubq", ubq, "mixed")
    perm = np.random.default_rng(16).permutation(F)
    assert (perm != np.arange(F)).sum() > F // 2
    a = ctx.sasa_ensemble(ubq, frames, "", PROBE, N_POINTS, per_frame=True)
    b = ctx.sasa_ensemble(ubq, frames[perm], "", PROBE, N_POINTS, per_frame=True)
    for k in SASA_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(b["count"], a["count"][perm]) and np.array_equal(bits(b["total_sasa"]), bits(a["total_sasa"][perm]))
    a = ctx.residue_sasa_ensemble(ubq, frames, "", PROBE, N_POINTS, "protor", per_frame=True)
    b = ctx.residue_sasa_ensemble(ubq, frames[perm], "", PROBE, N_POINTS, "protor", per_frame=True)
    for k in ("mean_sasa", "std_sasa", "min_sasa", "max_sasa", "mean_relative_sasa"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(bits(b["residue_sasa"]), bits(a["residue_sasa"][perm])) and np.array_equal(bits(b["chain_sasa"]), bits(a["chain_sasa"][perm]))
    a = ctx.dsasa_ensemble(ubq, frames, "/", PROBE, N_POINTS, per_frame=True)
    b = ctx.dsasa_ensemble(ubq, frames[perm], "/", PROBE, N_POINTS, per_frame=True)
    for k in ("sum_buried", "sum_buried_sq", "min_buried", "max_buried", "frames_buried"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(b["buried"], a["buried"][perm])
    for k in ("total_complex", "total_g1", "total_g2", "dsasa"):
        assert np.array_equal(bits(b[k]), bits(a[k][perm])), k
    for rings in (False, True):
        assert to_bytes(ctx.contact_frequencies(ubq, frames, "/", rings=rings)) == to_bytes(ctx.contact_frequencies(ubq, frames[perm], "/", rings=rings))


# ---- 6. the frame cap: 65 535 frames in a pass ---------------------------------------------------------------------------------------------------------
CAP_POINTS = 32


@pytest.fixture(scope="module")
def cap_case():
    rec = ts.cap_topology()
    conf = ts.cap_conformations(rec)
    return rec, aa.Structure.from_records(rec), conf, ts.cap_frames(conf), np.arange(ts.CAP_FRAMES) % ts.CAP_PERIOD


def test_frame_cap_sasa(big_ctx, cap_case):
    """The automatic pass is the model ordinal range: 65 535 frames, then six.  Expected: seven single calls and the restatement, tiled."""
    rec, s, conf, frames, idx = cap_case
    Fc = ts.CAP_FRAMES
    sph = aa.sasa_sphere_points(CAP_POINTS)
    got = big_ctx.sasa_ensemble(s, frames, "", PROBE, CAP_POINTS, per_frame=True)
    sel = got["atoms"].astype(np.int64)
    m = len(sel)
    assert m == len(rec["x"]) and 2 ** 21 / m > 65535 and got["n_frames"] == Fc == 65535 + 6
    loop = ec.frame_loop(big_ctx, s, sel, conf, PROBE, CAP_POINTS)
    for p in range(ts.CAP_PERIOD):
        x, y, z = xyz_of(conf[p], sel)
        assert np.array_equal(loop["count"][p], sr.atom_counts(x, y, z, loop["R"], sph)), p
    assert (loop["count"].min(0) != loop["count"].max(0)).any() and (loop["count"] < CAP_POINTS).any()
    want = {"count": loop["count"][idx], "sasa": loop["sasa"][idx]}
    assert_sasa_equal(got, want, loop["R"], CAP_POINTS)


def test_frame_cap_dsasa(big_ctx, cap_case):
    rec, s, conf, frames, idx = cap_case
    sph = aa.sasa_sphere_points(CAP_POINTS)
    got = big_ctx.dsasa_ensemble(s, frames, "A/B", PROBE, CAP_POINTS, per_frame=True)
    sel, mask = got["atoms"].astype(np.int64), got["group"]
    assert len(sel) == len(rec["x"]) and set(mask.tolist()) == {1, 2} and got["n_frames"] == ts.CAP_FRAMES
    loop = bsa_frame_loop(big_ctx, s, got, conf, PROBE, CAP_POINTS)
    for p in range(ts.CAP_PERIOD):
        x, y, z = xyz_of(conf[p], sel)
        assert np.array_equal(loop["buried"][p], bc.split_counts(x, y, z, got["R"], mask, sph)[1]), p
    assert (loop["buried"] > 0).any()
    assert np.array_equal(got["buried"], loop["buried"][idx])
    for k in ("total_complex", "total_g1", "total_g2", "dsasa"):
        assert np.array_equal(bits(got[k]), bits(loop[k][idx])), k
    b = loop["buried"][idx].astype(np.int64)
    assert np.array_equal(got["sum_buried"], b.sum(0).astype(np.uint64)) and np.array_equal(got["sum_buried_sq"], (b * b).sum(0).astype(np.uint64))
    assert np.array_equal(got["min_buried"], b.min(0)) and np.array_equal(got["max_buried"], b.max(0))
    assert np.array_equal(got["frames_buried"], (b > 0).sum(0).astype(np.uint32))


def test_frame_cap_contact_frequencies(big_ctx, cap_case):
    rec, s, conf, frames, idx = cap_case
    Fc, P = ts.CAP_FRAMES, ts.CAP_PERIOD
    assert 2 ** 21 / frames.shape[1] > 65535
    got = big_ctx.contact_frequencies(s, frames, "/")
    want = freq_expected(big_ctx, s, conf, "/")  # the rows of the seven conformations: identity, min and max distance over them
    key = lambda t: list(zip(t["from_atom"].tolist(), t["to_atom"].tolist(), t["interaction"].tolist()))  # noqa: E731
    times = np.bincount(idx, minlength=P)
    n_frames = dict.fromkeys(key(want), 0)
    for p in range(P):
        for k in key(freq_expected(big_ctx, s, conf[p:p + 1], "/")):
            n_frames[k] += int(times[p])
    cnt = np.array([n_frames[k] for k in key(want)], np.uint32)
    assert len(cnt) > 0 and (cnt == Fc).any() and (cnt < Fc).any() and int(times.sum()) == Fc
    want = dict(want, n_frames=cnt, frequency=(cnt.astype(np.float64) / Fc).astype(np.float32))
    assert_table_equal(got, want)
    a, b = rec["chain"] == b"A", rec["chain"] == b"B"
    across = a[got["from_atom"]] != a[got["to_atom"]]
    assert across.any() and b.any()  # the contact pair across the chains is in the table


# ---- 7. one-cell slabs over many frames ---------------------------------------------------------------------------------------------------------------
def test_flat_slabs_over_two_hundred_frames(ctx):
    """nx == ny == nz == 1: every frame is one cell and its separator.  The frames alternate between a buried and an open arrangement whose boxes
    overlap in box-relative coordinates; without the separator every open frame would be buried by its neighbours."""
    rec = ts.flat_topology()
    s = aa.Structure.from_records(rec)
    two, frames = ts.flat_arrangements(), ts.flat_frames()
    Ff = len(frames)
    idx = np.arange(Ff) % 2
    sph = aa.sasa_sphere_points(N_POINTS)
    got = ctx.sasa_ensemble(s, frames, "", PROBE, N_POINTS, per_frame=True)
    sel = got["atoms"].astype(np.int64)
    assert len(sel) == 4 and got["n_frames"] == Ff == 200
    R = (ec.vdw(s.strings("element")[sel]) + np.float32(PROBE)).astype(np.float32)
    counts = np.stack([sr.atom_counts(*xyz_of(two[p], sel), R, sph) for p in range(2)])
    assert (counts[0] < counts[1]).all() and (counts[1] < N_POINTS).any()  # buried, open -- and the open square still touches
    areas = np.stack([sr.sasa_from_counts(R, counts[p], N_POINTS) for p in range(2)])
    assert_sasa_equal(got, {"count": counts[idx], "sasa": areas[idx]}, R, N_POINTS)
    loop = ec.frame_loop(ctx, s, sel, two, PROBE, N_POINTS)
    assert np.array_equal(loop["count"], counts)
    for per in (67, 1):  # 67 + 67 + 66, and two hundred passes of one frame
        aa.debug_set("ens_chunk_atoms", per * 4)
        assert ec.result_bytes(ctx.sasa_ensemble(s, frames, "", PROBE, N_POINTS, per_frame=True)) == ec.result_bytes(got), per
    aa.debug_set("ens_chunk_atoms", 0)
    d = ctx.dsasa_ensemble(s, frames, "A/B", PROBE, N_POINTS, per_frame=True)
    buried = np.stack([bc.split_counts(*xyz_of(two[p], d["atoms"].astype(np.int64)), d["R"], d["group"], sph)[1] for p in range(2)])
    assert np.array_equal(d["buried"], buried[idx]) and (buried[0] > buried[1]).all()
    assert np.array_equal(d["frames_buried"], ((buried[idx] > 0).sum(0)).astype(np.uint32))
