"""The cases of tests/test_ens_shapes_gpu.py reach what they are named for (CPU; tests/trajectory_shapes.py holds the generators and the
restatement of grid.inl grid_setup's sizing loop).  These are conditions, not measurements: a factor that misses its condition is changed,
never the assertion."""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import ens_sasa_common as ec
import residue_sasa_common as rc
import trajectory_shapes as ts
from conftest import DATA

F = 16
PROBE = 1.4
SAP_RADIUS = 10.0


def sasa_cutoff(r_max: float) -> float:
    return 2.0 * float(r_max) * (1.0 + 1e-5) + 1e-6  # sasa_dev.cpp sasa_cutoff


@pytest.fixture(scope="module")
def ubq():
    s = aa.load_model(str(DATA / "1ubq.pdb"))
    sel = aa.sasa_select(s).astype(np.int64)
    R = (ec.vdw(s.strings("element")[sel]) + np.float32(PROBE)).astype(np.float32)
    Rp = (rc.table_radii(s, sel, "protor")[0] + np.float32(PROBE)).astype(np.float32)
    side = ~np.isin(s.strings("atomn")[sel], ec.BACKBONE)
    return {"s": s, "base": ec.topology_xyz(s), "sel": sel, "R": R, "R_protor": Rp, "side": side}


@pytest.fixture(scope="module")
def bft_hl():
    s = aa.load_model(str(DATA / "6bft.pdb"))
    return ec.topology_xyz(s), aa.sasa_select(s, "H,L").astype(np.int64)


def sizings(u, frames, per=None):
    """(SASA grid, SAP grid) of the pass that holds the first `per` frames.  The cell capacity is that of the largest workspace a context that
    only ever runs these 16-frame cases can hold: contact_frequencies packs all the topology's atoms, not only the selected ones."""
    cap = ts.cell_capacity(F * len(u["base"]))
    m = len(u["sel"])
    sasa = ts.sizing_of(frames[:, u["sel"]], m, sasa_cutoff(u["R"].max()), f32_coordinates=True, per=per, ncells_cap=cap)
    sap = ts.sizing_of(frames[:, u["sel"][u["side"]]], m, SAP_RADIUS, per=per, ncells_cap=cap)
    return sasa, sap


def test_the_capacity_formula_is_the_engines():
    """engine.cpp ensure_workspace: cap = max(n + n / 8, 1024) atoms, 8 cap + 65536 cells."""
    src = (DATA.parent.parent / "arpeggia_amd" / "csrc" / "engine.cpp").read_text()
    assert "std::max<uint64_t>(n + n / 8, 1024)" in src and "std::min<uint64_t>(8 * cap + 65536, 0xFFFFFFF0ull)" in src
    assert ts.cell_capacity(0) == 8 * 1024 + 65536 and ts.cell_capacity(9632) == 8 * (9632 + 1204) + 65536
    grid = (DATA.parent.parent / "arpeggia_amd" / "csrc" / "grid.inl").read_text()
    assert "edge *= 1.2599210498948732;" in grid and "g->nzt = nm * (g->nz + 1u);" in grid


def test_generators_are_deterministic_and_shaped(ubq):
    for name in ts.SHAPES:
        a, ea = ts.make(name, ubq["base"], F)
        b, eb = ts.make(name, ubq["base"], F)
        assert a.shape == (F,) + ubq["base"].shape and a.dtype == np.float64 and np.array_equal(a, b) and ea == eb and np.isfinite(a).all(), name
        assert all(0 <= v < F for v in ea.values()) and len(np.unique(a.reshape(F, -1), axis=0)) == F, name
        assert ts.forced_passes(name, F)[:2] == [6, 1]
    assert ts.forced_passes("swell@last", F) == [6, 1, 15] and ts.forced_passes("collapse@last", F) == [6, 1, 15]  # 15 + 1: the last frame alone


def test_drift_reaches_f32_spacing_and_keeps_one_frame(ubq):
    frames, ex = ts.make("drift", ubq["base"], F)
    assert np.array_equal(frames[ex["home"]], ubq["base"])
    shift = frames[:, 0] - ubq["base"][0]
    norms = np.linalg.norm(shift, axis=1)
    assert norms[0] == 0.0 and (np.diff(norms) > 0).all() and norms[-1] >= 1e5
    assert shift[-1, 0] > 0 > shift[-1, 1] and shift[-1, 2] > 0  # mixed signs
    far = frames[ex["far"]][ubq["sel"]]
    assert ts.f32_spacing(far).min() >= 2.0 ** -8
    # the records of the far frame against a midpoint shared with frame 0 would carry that spacing: far more than the kernels' f32 bands allow
    sasa, sap = sizings(ubq, frames)
    assert sasa["steps"] == 0 and sap["steps"] == 0  # a drifting trajectory costs no more cells than an aligned one
    aligned = sizings(ubq, np.repeat(ubq["base"][None], F, 0))
    assert abs(sasa["nx"] - aligned[0]["nx"]) <= 1 and abs(sasa["nz"] - aligned[0]["nz"]) <= 1


def test_tumble_takes_its_extents_from_different_frames(ubq, bft_hl):
    frames, _ = ts.make("tumble", ubq["base"], F)
    assert len(set(ts.axis_owners(frames[:, ubq["sel"]], True))) >= 2
    base, sel = bft_hl
    frames = ts.tumble(base, 8)
    owners = ts.axis_owners(frames[:, sel], True)
    assert len(set(owners)) >= 2
    ext = ts.frame_extents(frames[:, sel], True)
    assert (ext.max(0) > 1.15 * np.median(ext, 0)).all()  # an elongated topology: one frame's box is too small for the others on every axis
    # rigid: every distance kept
    d0 = np.linalg.norm(base[sel][:50, None] - base[sel][None, :50], axis=-1)
    assert all(np.allclose(np.linalg.norm(fr[sel][:50, None] - fr[sel][None, :50], axis=-1), d0, atol=1e-9) for fr in frames)


@pytest.mark.parametrize("name", [n for n in ts.SHAPES if n.startswith("swell")] + ["mixed"])
def test_swell_coarsens_both_grids(ubq, name):
    frames, ex = ts.make(name, ubq["base"], F)
    sasa, sap = sizings(ubq, frames)
    assert sasa["steps"] >= 1 and sap["steps"] >= 1, (sasa, sap)
    assert sasa["nx"] * sasa["ny"] * sasa["nzt"] <= sasa["cap"] and sasa["edge"] > sasa_cutoff(ubq["R"].max())
    # one frame is what does it: without it nothing coarsens
    others = np.delete(frames, ex["swollen"], 0)
    if name != "mixed":
        a, b = sizings(ubq, others)
        assert a["steps"] == 0 and b["steps"] == 0


def test_stretch_keeps_its_neighbours_at_large_record_coordinates(ubq):
    frames, ex = ts.make("stretch@mid", ubq["base"], F)
    f, sel = ex["stretched"], ubq["sel"]
    ext = ts.frame_extents(frames[:, sel], True)
    assert ts.axis_owners(frames[:, sel], True) == [f, f, f] and (ext[f] > 200.0 * np.median(ext, 0)).all()
    # against the frame's own midpoint its records are about ext / 2: f32 steps of 2^-11 A and more on every axis ...
    assert (ts.f32_spacing(ext[f] / 2.0) >= 2.0 ** -11).all()
    # ... and, unlike the swollen frame, every atom still has neighbours to be tested against there
    for R in (ubq["R"], ubq["R_protor"]):
        near = ts.pair_counts_within(frames[f][sel], R)
        assert near.min() >= 1 and np.median(near) > 15
    sasa, sap = sizings(ubq, frames)
    assert sasa["steps"] >= 1 and sap["steps"] >= 1


@pytest.mark.parametrize("axes", ["z", "yz", "xyz"])
def test_flat_frames_make_one_layer_slabs(ubq, axes):
    frames, _ = ts.make("flat_" + axes, ubq["base"], F)
    ext = ts.frame_extents(frames[:, ubq["sel"]])
    k = ["xyz".index(a) for a in axes]
    # (an f64 coordinate that is no f32 value gets a box one f32 step wide: the box codes are rounded outwards)
    assert (ext[0::2][:, k] <= 4e-6).all() and (ext[1::2][:, k] > 0.25).all() and (ext[:, k] <= 0.51).all()
    assert (ts.frame_extents(frames[:, ubq["sel"]], True)[0::2][:, k] == 0.0).all()
    for g in sizings(ubq, frames):
        assert g["nz"] == 1 and g["nzt"] == 2 * F and g["steps"] == 0
        assert ("y" not in axes or g["ny"] == 1) and ("x" not in axes or g["nx"] == 1)
    for per in (6, 1):  # the forced passes as well
        assert all(g["nz"] == 1 for g in sizings(ubq, frames, per))


@pytest.mark.parametrize("name", [n for n in ts.SHAPES if n.startswith(("collapse", "point"))] + ["mixed"])
def test_collapse_fills_the_list(ubq, name):
    frames, ex = ts.make(name, ubq["base"], F)
    m = len(ubq["sel"])
    for label in ("collapsed", "point"):
        if label in ex:
            for R in (ubq["R"], ubq["R_protor"]):
                near = ts.pair_counts_within(frames[ex[label]][ubq["sel"]], R)
                assert near.min() == m - 1 > 256  # every selected atom is a neighbour of every other: more than 256 list entries, k_sasa flushes
    if "point" in ex:
        assert len(np.unique(frames[ex["point"]], axis=0)) == 1
    assert ts.REACH < 2.0 * float(min(ubq["R"].min(), ubq["R_protor"].min()))


def test_the_frame_cap_case_hits_the_cap():
    rec = ts.cap_topology()
    n = len(rec["x"])
    assert n <= 31 and len(set(rec["chain"].tolist())) == 2 and len(set(zip(rec["chain"].tolist(), rec["resi"].tolist()))) == 3
    assert ts.AUTO_PASS_ATOMS / n > 65535 and ts.CAP_FRAMES == 65535 + 6
    conf = ts.cap_conformations(rec)
    assert conf.shape == (ts.CAP_PERIOD, n, 3) and len(np.unique(conf.reshape(ts.CAP_PERIOD, -1), axis=0)) == ts.CAP_PERIOD
    frames = ts.cap_frames(conf, 30)
    assert np.array_equal(frames[7], frames[0]) and not np.array_equal(frames[1], frames[0])
    # a contact pair across the chains in every conformation, and the boxes overlap where they are
    a, b = rec["chain"] == b"A", rec["chain"] == b"B"
    for c in conf:
        assert np.linalg.norm(c[a][:, None] - c[b][None], axis=-1).min() < 3.9
    lo, hi = conf.min(1), conf.max(1)
    assert (lo.max(0) < hi.min(0)).all()
    # one pass of 65 535 frames fits the cells it needs without coarsening: 2 layers per frame
    g = ts.grid_sizing(ts.frame_extents(conf).max(0), 65535, 65535 * n, sasa_cutoff(1.7 + 1.4))
    assert g["steps"] == 0 and g["nzt"] == 65535 * (g["nz"] + 1) and g["nx"] * g["ny"] * g["nzt"] <= g["cap"]


def test_the_flat_slab_case_is_one_cell_per_frame():
    rec = ts.flat_topology()
    frames = ts.flat_frames()
    assert 3 <= len(rec["x"]) <= 8 and frames.shape == (200, 4, 3) and np.array_equal(frames[0], frames[2]) and not np.array_equal(frames[0], frames[1])
    ext = ts.frame_extents(frames, True).max(0)
    for per in (200, 67, 1):
        g = ts.grid_sizing(ext, per, per * 4, sasa_cutoff(1.7 + 1.4))
        assert (g["nx"], g["ny"], g["nz"], g["steps"]) == (1, 1, 1, 0) and g["nzt"] == 2 * per
    buried, open_ = ts.flat_arrangements()
    d = lambda c: np.linalg.norm(c[:, None] - c[None], axis=-1)[np.triu_indices(4, 1)]  # noqa: E731
    assert d(buried).max() < 1.7 and d(open_).min() > 5.4
