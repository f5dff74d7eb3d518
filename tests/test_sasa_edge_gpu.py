"""k_sasa (arpeggia_amd/csrc/sasa.inl: the plain instantiation of sasa_walk) where the rest of the suite does not reach: the flush of the 256-entry neighbour list, the strict edge
d^2 < R_j^2 at point 0, placements within a few f32 steps of a neighbour's sphere, 64 passes of points, heterogeneous and zero radii, include
masks, large extents, and the same kernel under the ensemble path and dSASA.  Everything is compared as integers and f32 bit patterns with the
restatement of the contract (tests/sasa_restatement.py), which tests/test_sasa_edge_host.py holds to exact rational arithmetic on these very
cases, and where it is cheap with the rationals themselves (tests/sasa_edge_cases.py).  Nothing here is approximate.

ARP_FUZZ_SASA_DRAWS: draws of the near-sphere family (default 300, x 7 placements each)."""
import os

import numpy as np
import pytest

import arpeggia_amd as aa
import ens_sasa_common as ens
import sasa_edge_cases as edge
import sasa_restatement as sr
import synth
from arpeggia_amd import _lib
from conftest import DATA

pytestmark = pytest.mark.gpu

N_DRAWS = int(os.environ.get("ARP_FUZZ_SASA_DRAWS", "300"))
NEAR_POINTS = 24


@pytest.fixture(scope="module")
def ctx():
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


def _vdw(elements) -> np.ndarray:
    p = aa.default_params()
    return np.array([p.vdw_radius[_lib.lib.arp_element_class(e)] for e in elements], dtype=np.float32)


_structures = {}


def structure_inputs(name: str):
    if name not in _structures:
        s = aa.load_model(str(DATA / f"{name}.pdb"))
        sel, soa = aa.sasa_select(s), s.soa()
        _structures[name] = (soa["x"][sel], soa["y"][sel], soa["z"][sel], _vdw(s.strings("element")[sel]))
    return _structures[name]


def check(ctx, x, y, z, r, probe, n_points=100, homes=None, include=None):
    """One device call against the restatement: counts and SASA bits of `homes` (positions among the included atoms; default all of them);
    atoms outside `include` must come back as zeros.  Returns the device counts."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    r = np.asarray(r, np.float32)
    sasa, count = aa.atom_sasa(ctx, x, y, z, r, include=include, probe=probe, n_points=n_points)
    inc = np.arange(len(x)) if include is None else np.flatnonzero(include)
    if include is not None:
        out = np.setdiff1d(np.arange(len(x)), inc)
        assert (count[out] == 0).all() and (sasa[out].view(np.uint32) == 0).all()
    R = (r[inc] + np.float32(probe)).astype(np.float32)
    want = sr.atom_counts(x[inc], y[inc], z[inc], R, aa.sasa_sphere_points(n_points), homes=homes, chunk_pairs=max(64, 4_000_000 // n_points))
    at = inc if homes is None else inc[np.asarray(homes)]
    assert count.dtype == np.int32 and np.array_equal(count[at], want), int((count[at] != want).sum())
    want_sasa = sr.sasa_from_counts(R if homes is None else R[np.asarray(homes)], want, n_points)
    assert np.array_equal(sasa[at].view(np.uint32), want_sasa.view(np.uint32))
    assert 0 <= count.min() and count.max() <= n_points
    return count


# ---- the neighbour-list flush -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", [4.0, 5.0, 8.0, 12.0])
@pytest.mark.parametrize("name", ["1ubq", "6bft"])
def test_flush_on_structures_at_large_probes(ctx, name, probe):
    x, y, z, r = structure_inputs(name)
    nb = edge.neighbour_counts(x, y, z, (r + np.float32(probe)).astype(np.float32))
    assert nb.max() > 256  # (how far above, and that points stay open: tests/test_sasa_edge_host.py)
    homes = None if name == "1ubq" else edge.homes_sample(nb, 32, 96)
    count = check(ctx, x, y, z, r, probe, homes=homes)
    if probe in (5.0, 8.0):
        assert (count[nb > 256] > 0).any()


def test_flush_on_a_dense_cloud(ctx):
    rec = synth.gen_s1(40_000)
    r = _vdw(rec["element"])
    nb = edge.neighbour_counts(rec["x"], rec["y"], rec["z"], (r + np.float32(5.0)).astype(np.float32))
    assert (nb > 256).sum() > 20_000
    count = check(ctx, rec["x"], rec["y"], rec["z"], r, 5.0, homes=edge.homes_sample(nb, 32, 224))
    assert (count[nb > 256] > 0).any()


@pytest.mark.parametrize("n_points", [100, 128])
@pytest.mark.parametrize("n", [300, 600, 1100])
def test_flush_on_coincident_atoms(ctx, n, n_points):
    """Every test of every point sits within rounding of d^2 = R^2: the f64 band and the flush act together (1100 atoms: four flushes)."""
    x, y, z, r = edge.coincident(n)
    count = check(ctx, x, y, z, r, 0.0, n_points, homes=np.array([0, n // 2, n - 1]))
    assert (count == count[0]).all() and 0 < count[0] < n_points  # every atom sees n - 1 copies of the same neighbour
    assert count[0] == check(ctx, x[:2], y[:2], z[:2], r[:2], 0.0, n_points)[0]  # as many open points as against one copy


# ---- the strict edge at point 0 and placements near the sphere ---------------------------------------------------------------------------------
def test_on_axis_point_zero_is_the_strict_edge(ctx):
    cases = edge.on_axis_cases()
    touching = 0
    for n_points in (1, 64, 100):
        sphere = aa.sasa_sphere_points(n_points)
        assert sphere[0].tolist() == [0.0, 0.0, 1.0]
        for c in cases:
            count = check(ctx, c["x"], c["y"], c["z"], c["radius"], c["probe"], n_points)
            if n_points == 1:
                home, m = c["home"], c["margin"]
                assert count[home] == (0 if m < 0 else 1) and count[1 - home] == 1, c
                if c["representable"]:  # d^2 == R_j^2: open; one f32 step closer: buried
                    assert count.tolist() == ([1, 1] if c["step"] >= 0 else ([1, 0] if c["swap"] else [0, 1])), c
                    touching += c["touch"]
    assert touching >= 30


def test_placements_within_three_f32_steps_of_the_sphere(ctx):
    sphere = aa.sasa_sphere_points(NEAR_POINTS)
    placements = edge.near_sphere_placements(sphere, N_DRAWS)
    left_out = 0
    for p in placements:  # alone: a small box, the narrow band
        c = p["c"].astype(np.float64)
        count = check(ctx, c[:, 0], c[:, 1], c[:, 2], p["R"], 0.0, NEAR_POINTS)
        want, undecided = edge.exact_pair_counts(p["c"], p["R"], sphere)
        left_out += undecided
        assert count.tolist() == want, (p["draw"], p["step"])
    assert left_out == 0
    for name, c, R, ps in edge.placement_batches(placements):  # in company: boxes of hundreds and of 10^4..10^5 A, the wide band
        c = c.astype(np.float64)
        check(ctx, c[:, 0], c[:, 1], c[:, 2], R, 0.0, NEAR_POINTS)


# ---- points: up to 64 passes, bit 63 of the per-lane word --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", [128, 2049, 4095, 4096])
@pytest.mark.parametrize("probe", [1.4, 5.0])
def test_many_points_on_1ubq(ctx, n_points, probe):
    x, y, z, r = structure_inputs("1ubq")
    nb = edge.neighbour_counts(x, y, z, (r + np.float32(probe)).astype(np.float32))
    assert (nb.max() > 256) == (probe == 5.0)
    homes = None if n_points == 128 else edge.homes_sample(nb, 8, 24 if probe == 5.0 else 72)
    count = check(ctx, x, y, z, r, probe, n_points, homes=homes)
    assert count.max() > 0


# ---- radii ----------------------------------------------------------------------------------------------------------------------------------
def test_radii_from_zero_to_twelve_over_a_cloud(ctx):
    rec = synth.gen_s1(20_000)
    r = np.random.default_rng(5).uniform(0.0, 12.0, len(rec["x"])).astype(np.float32)
    r[:50] = 0.0
    homes = np.unique(np.concatenate([np.argsort(-r, kind="stable")[:16], np.arange(8), np.random.default_rng(6).choice(len(r), 120, replace=False)]))
    count = check(ctx, rec["x"], rec["y"], rec["z"], r, 0.0, homes=homes)
    assert (count > 0).any() and (count == 0).any()


def test_one_huge_atom_among_forty_thousand(ctx):
    """r_max sets the cell edge: every wave scans thousands of slots and only the per-neighbour R_j bound cuts them."""
    rec = synth.gen_s1(40_000)
    x, y, z = rec["x"], rec["y"], rec["z"]
    r = _vdw(rec["element"])
    c = np.stack([x, y, z], 1)
    big = int(np.argmin(((c - c.mean(0)) ** 2).sum(1)))
    r[big] = 30.0
    d = np.sqrt(((c - c[big]) ** 2).sum(1))
    homes = np.unique(np.concatenate([[big], np.argsort(np.abs(d - 31.4), kind="stable")[:40], np.random.default_rng(8).choice(len(r), 60, replace=False)]))
    count = check(ctx, x, y, z, r, 1.4, homes=homes)
    inside = (d < 25.0) & (np.arange(len(r)) != big)
    assert inside.sum() > 1000 and (count[inside] == 0).all() and (count[d > 40.0] > 0).any()


@pytest.mark.parametrize("n_points", [1, 100, 4096])
def test_all_radii_zero_with_probe_zero(ctx, n_points):
    x, y, z, r = structure_inputs("1ubq")
    x, y, z = (np.concatenate([v, v[:7]]) for v in (x, y, z))  # with coincident atoms: d^2 = 0 < 0 is false
    zero = np.zeros(len(x), np.float32)
    sasa, count = aa.atom_sasa(ctx, x, y, z, zero, probe=0.0, n_points=n_points)
    assert (count == n_points).all() and (sasa.view(np.uint32) == 0).all()
    check(ctx, x, y, z, zero, 0.0, n_points, homes=np.arange(0, len(x), 9))


@pytest.mark.parametrize("probe,n_atoms", [(1.4, 40_000), (5.0, 10_000)])
def test_random_include_masks_on_clouds(ctx, probe, n_atoms):
    rec = synth.gen_s1(n_atoms)
    r = _vdw(rec["element"])
    rng = np.random.default_rng(int(probe * 10))
    include = (rng.random(len(r)) < 0.5).astype(np.uint8)
    r[include == 0] = np.float32(50.0)  # the radius of an excluded atom must not matter, not even as the largest
    homes = np.sort(rng.choice(int(include.sum()), 1500 if probe == 1.4 else 200, replace=False))
    check(ctx, rec["x"], rec["y"], rec["z"], r, probe, homes=homes, include=include)


def test_include_mask_on_a_flush_input(ctx):
    x, y, z, r = structure_inputs("6bft")
    include = (np.random.default_rng(3).random(len(r)) < 0.7).astype(np.uint8)
    inc = np.flatnonzero(include)
    nb = edge.neighbour_counts(x[inc], y[inc], z[inc], (r[inc] + np.float32(6.0)).astype(np.float32))
    assert nb.max() > 300
    check(ctx, x, y, z, r, 6.0, homes=edge.homes_sample(nb, 24, 72), include=include)


# ---- extents ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", [1.4, 5.0])
def test_two_clusters_a_hundred_thousand_angstrom_apart(ctx, probe):
    """C of the band width grows with the box: every test of both clusters goes through the f64 branch."""
    x, y, z, r = structure_inputs("1ubq")
    far = np.array([1.0e5, -3.0e4, 250.0])
    check(ctx, np.concatenate([x, x + far[0]]), np.concatenate([y, y + far[1]]), np.concatenate([z, z + far[2]]), np.concatenate([r, r]), probe)


@pytest.mark.parametrize("shift", [(9000.0, -9000.0, 9000.0), (0.0, 0.0, -9000.0)])
def test_structure_translated_by_nine_thousand_angstrom(ctx, shift):
    x, y, z, r = structure_inputs("1ubq")
    count = check(ctx, x + shift[0], y + shift[1], z + shift[2], r, 1.4)
    assert (count > 0).any()


# ---- the same kernel under the ensemble path and dSASA ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1ubq", "6bft"])
def test_flush_under_the_ensemble_path(ctx, name):
    s = aa.load_model(str(DATA / f"{name}.pdb"))
    frames = ens.jittered(s, 3, seed=41)
    try:
        got = ctx.sasa_ensemble(s, frames, "", 6.0, 100, per_frame=True)
        sel = got["atoms"]
        m = len(sel)
        for budget in (m, 2 * m):  # one and two frames per pass
            aa.debug_set("ens_chunk_atoms", budget)
            assert ens.result_bytes(ctx.sasa_ensemble(s, frames, "", 6.0, 100, per_frame=True)) == ens.result_bytes(got), budget
    finally:
        aa.debug_set("ens_chunk_atoms", 0)
    loop = ens.frame_loop(ctx, s, sel, frames, 6.0, 100)
    assert np.array_equal(got["count"], loop["count"])
    sphere = aa.sasa_sphere_points(100)
    for f in range(len(frames)):
        x, y, z = (np.ascontiguousarray(frames[f][sel, k]) for k in range(3))
        nb = edge.neighbour_counts(x, y, z, loop["R"])
        assert (nb > 256).sum() > 100
        homes = np.arange(m) if name == "1ubq" else edge.homes_sample(nb, 16, 48)
        want = sr.atom_counts(x, y, z, loop["R"], sphere, homes=homes)
        assert np.array_equal(got["count"][f][homes], want)
    assert (got["count"] > 0).any()


def test_dsasa_on_6bft_at_probe_five(ctx):
    """include/arpeggia_amd.h arp_structure_dsasa: complex, group 1 and group 2 each summed in f64 in atom order and rounded to f32 once;
    f32(g1 + g2) - complex in f32."""
    s = aa.load_model(str(DATA / "6bft.pdb"))
    n_points, probe = 100, 5.0
    got = aa.get_dsasa(s, "C/H,L", probe_radius=probe, n_points=n_points)
    soa, sphere = s.soa(), aa.sasa_sphere_points(n_points)
    totals = []
    for chains in ("C,H,L", "C", "H,L"):
        sel = aa.sasa_select(s, chains)  # (a single-model file: steps 2-4 select what steps 1-5 do)
        assert len(sel) > 500
        R = (_vdw(s.strings("element")[sel]) + np.float32(probe)).astype(np.float32)
        counts = sr.atom_counts(soa["x"][sel], soa["y"][sel], soa["z"][sel], R, sphere)
        totals.append(np.float32(np.cumsum(sr.sasa_from_counts(R, counts, n_points).astype(np.float64))[-1]))
    want = np.float32(np.float32(totals[1] + totals[2]) - totals[0])
    assert np.float32(got).view(np.uint32) == want.view(np.uint32), (got, want)
    assert want > 100.0


def test_the_kernel_did_run_tests(ctx):
    x, y, z, r = structure_inputs("1ubq")
    aa.atom_sasa(ctx, x, y, z, r, probe=8.0)
    assert aa.sasa_tests(ctx) > 100 * len(x)
