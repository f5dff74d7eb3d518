"""CPU checks behind tests/test_sasa_edge_gpu.py and tests/test_sap_sum_edge_gpu.py: the restatement of the SASA contract
(tests/sasa_restatement.py) against exact rational arithmetic on the generated edge cases, and the preconditions of the device inputs --
a device test must not be able to pass without reaching the path it is there for.  No compute call is made."""
import numpy as np
import pytest

import arpeggia_amd as aa
import sasa_edge_cases as ec
import sasa_restatement as sr
import synth
from arpeggia_amd import _lib
from conftest import DATA

N_POINTS = 24  # of the near-sphere family here: every point of both atoms goes through the rationals


def _vdw(elements) -> np.ndarray:
    p = aa.default_params()
    return np.array([p.vdw_radius[_lib.lib.arp_element_class(e)] for e in elements], dtype=np.float32)


def structure_inputs(name: str):
    s = aa.load_model(str(DATA / f"{name}.pdb"))
    sel, soa = aa.sasa_select(s), s.soa()
    return soa["x"][sel], soa["y"][sel], soa["z"][sel], _vdw(s.strings("element")[sel])


def test_exact_margin_on_hand_cases():
    up = (0.0, 0.0, 1.0)
    assert ec.exact_margin((0, 0, 0), (0, 0, 6), up, 3.0, 3.0) == 0
    assert ec.exact_margin((0, 0, 0), (0, 0, 5), up, 3.0, 3.0) == -5 and ec.exact_margin((0, 0, 0), (0, 0, 7), up, 3.0, 3.0) == 7
    # from the f32 values of the arguments: 0.1 is not 1/10
    m = ec.exact_margin((0.1, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0.0)
    assert m == ec.Fraction(float(np.float32(0.1))) ** 2 and m != ec.Fraction(1, 100)
    assert not ec.decided(ec.Fraction(0), 3.0) and ec.decided(ec.Fraction(1, 2 ** 36), 3.0) and not ec.decided(ec.Fraction(9, 2 ** 40), 3.0)


def test_restatement_equals_exact_arithmetic_near_the_sphere():
    """Every point of both atoms of every placement: restatement == rationals; nothing is left out."""
    sphere = sr.sphere_points(N_POINTS)
    placements = ec.near_sphere_placements(sphere)
    assert len(placements) == 2100 and {p["offset"] for p in placements} == set(ec.OFFSETS)
    left_out, smallest = 0, None
    for p in placements:
        want, undecided = ec.exact_pair_counts(p["c"], p["R"], sphere)
        left_out += undecided
        got = sr.atom_counts(p["c"][:, 0], p["c"][:, 1], p["c"][:, 2], p["R"], sphere)
        assert got.tolist() == want, (p["draw"], p["step"])
        rel = abs(p["margin"]) / ec.Fraction(float(p["R"][1])) ** 2
        smallest = rel if smallest is None else min(smallest, rel)
    assert left_out == 0
    # the placements do sit on the sphere: the designated point is within a few f32 steps of R_j^2, on both sides of it
    rel = np.array([float(p["margin"] / ec.Fraction(float(p["R"][1])) ** 2) for p in placements])
    at_origin = np.array([p["offset"] == 0.0 for p in placements])
    assert np.abs(rel[at_origin]).max() < 1e-3 and np.abs(rel).max() < 0.05  # (an f32 step at 500 A is 3 x 10^-5 A, at 50 000 A 4 x 10^-3 A)
    assert (rel < 0).sum() > 500 and (rel > 0).sum() > 500
    assert float(smallest) > 2.0 ** -40


def test_placement_batches_hold_every_placement_once_per_kind():
    sphere = sr.sphere_points(N_POINTS)
    placements = ec.near_sphere_placements(sphere)
    batches = ec.placement_batches(placements)
    assert len(batches) == 7 * 5
    assert sum(len(ps) for name, _, _, ps in batches if name.startswith("offset")) == len(placements)
    assert sum(len(ps) for name, _, _, ps in batches if name.startswith("mixed")) == len(placements)
    for name, c, R, ps in batches:
        extent = float((c.max(0) - c.min(0)).max())
        assert (extent > 5.0e4) if name.startswith("mixed") else (extent < 1000.0), name
        got = sr.atom_counts(c[:, 0], c[:, 1], c[:, 2], R, sphere)
        for k, p in enumerate(ps):  # in company or alone: the same counts
            assert got[2 * k:2 * k + 2].tolist() == sr.atom_counts(p["c"][:, 0], p["c"][:, 1], p["c"][:, 2], p["R"], sphere).tolist()


def test_on_axis_point_zero_is_the_strict_edge():
    cases = ec.on_axis_cases()
    assert sum(c["touch"] for c in cases) >= 2 * 15 and any(c["touch"] and c["z"].max() > 4.0e4 for c in cases)
    assert any(not c["representable"] for c in cases)
    for n_points in (1, 64, 100):
        sphere = sr.sphere_points(n_points)
        assert sphere[0].tolist() == [0.0, 0.0, 1.0]
        assert not ((sphere[:, 1] == 0.0) & (sphere[:, 2] == 0.0)).any()  # no point on the x axis: two atoms along x never touch at a point
        for c in cases:
            home, other = c["home"], 1 - c["home"]
            got = sr.atom_counts(c["x"], c["y"], c["z"], c["R"], sphere)
            m = c["margin"]
            assert m == 0 if c["touch"] else m != 0
            if c["representable"]:  # exactly touching: open; one f32 step closer: buried; one step farther: open
                assert (m < 0) == (c["step"] == -1)
            assert ec.decided(m, c["R"][other]) or m == 0
            if n_points == 1:
                assert got[home] == (0 if m < 0 else 1) and got[other] == 1, c
                if c["representable"]:
                    assert got.tolist() == ([1, 1] if c["step"] >= 0 else ([1, 0] if c["swap"] else [0, 1]))
            else:
                c2 = np.stack([ec.f32(c["x"]), ec.f32(c["y"]), ec.f32(c["z"])], 1)
                want, undecided = ec.exact_pair_counts(c2, c["R"], sphere)
                assert (undecided == 0 or c["touch"]) and got.tolist() == want


def test_coincident_atoms_sit_on_the_edge_and_exact_arithmetic_decides():
    x, y, z, r = ec.coincident(2)
    for n_points in (100, 128):
        sphere = sr.sphere_points(n_points)
        c = np.stack([ec.f32(x), ec.f32(y), ec.f32(z)], 1)
        want, undecided = ec.exact_pair_counts(c, r, sphere)
        margins = [ec.exact_margin(c[0], c[1], s, r[0], r[1]) for s in sphere]
        # the pole (0, 0, 1) gives d^2 == R^2 in exact and in f64 arithmetic alike (not buried); every other point is decided
        assert undecided == 2 and margins[0] == 0 and all(ec.decided(m, r[1]) for m in margins[1:])
        got = sr.atom_counts(x, y, z, r, sphere)
        assert got.tolist() == want and 0 < want[0] < n_points  # some |s_k|^2 round below 1, some do not
        assert max(abs(float(m)) for m in margins) / float(r[1]) ** 2 < 1e-6


# ---- preconditions of the flush inputs --------------------------------------------------------------------------------------------------
def _open_points_of_crowded_atoms(x, y, z, R, nb, above: int):
    """Counts of the atoms with more than `above` neighbours that have the fewest of them (the likeliest to keep open points)."""
    crowded = np.flatnonzero(nb > above)
    homes = np.sort(crowded[np.argsort(nb[crowded], kind="stable")[:48]])
    return sr.atom_counts(x, y, z, R, sr.sphere_points(100), homes=homes)


@pytest.mark.parametrize("name,probe,above", [("1ubq", 4.0, 256), ("1ubq", 5.0, 256), ("1ubq", 8.0, 512), ("1ubq", 12.0, 512),
                                              ("6bft", 4.0, 256), ("6bft", 5.0, 256), ("6bft", 8.0, 512), ("6bft", 12.0, 1024)])
def test_structures_at_large_probes_fill_the_neighbour_list(name, probe, above):
    x, y, z, r = structure_inputs(name)
    R = (r + np.float32(probe)).astype(np.float32)
    nb = ec.neighbour_counts(x, y, z, R)
    assert (nb > above).sum() >= 30, int(nb.max())
    if probe in (5.0, 8.0):  # a flush with points still open: the buried bits must survive it (at probe 4 and 12 the crowded atoms are buried)
        assert (nb > 256).any() and (_open_points_of_crowded_atoms(x, y, z, R, nb, 256) > 0).any()
    homes = ec.homes_sample(nb, 16, 32)
    assert nb.max() in nb[homes] and len(np.unique(homes)) == 48


def test_dense_cloud_and_coincident_atoms_fill_the_neighbour_list():
    rec = synth.gen_s1(40_000)
    R = (_vdw(rec["element"]) + np.float32(5.0)).astype(np.float32)
    nb = ec.neighbour_counts(rec["x"], rec["y"], rec["z"], R)
    assert (nb > 256).sum() > 20_000 and nb.max() > 400
    assert (_open_points_of_crowded_atoms(rec["x"], rec["y"], rec["z"], R, nb, 256) > 0).any()
    for n, above in ((300, 256), (600, 512), (1100, 1024)):
        x, y, z, r = ec.coincident(n)
        nb = ec.neighbour_counts(x, y, z, r)
        assert (nb == n - 1).all() and n - 1 > above
        assert (sr.atom_counts(x, y, z, r, sr.sphere_points(100), homes=np.array([0, n - 1])) > 0).all()


# ---- preconditions of the neighbour-sum inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in ec.SUM_CLOUDS])
def test_sum_clouds_are_exact_and_sit_on_the_edge(name):
    _, n, lattice, side, radii = ec.SUM_CLOUDS[[c[0] for c in ec.SUM_CLOUDS].index(name)]
    cloud = ec.sum_cloud(name)
    assert (n >= ec.SPLIT3_FROM) == ("230k" in name) and len(cloud["x"]) == n
    q = cloud["q"]
    assert q.min() >= 0 and q.max() < 4096 * ec.SCALE
    assert np.array_equal(np.stack([cloud["x"], cloud["y"], cloud["z"]], 1) * ec.SCALE, q.astype(np.float64))
    w8 = cloud["w"].astype(np.float64) * 8.0
    assert np.array_equal(w8, np.round(w8)) and np.abs(w8).max() == 8.0 and (w8 == 0).any() and (w8 < 0).any() and not cloud["side"].all()
    cand = ec.candidate_pairs(cloud, radii[0])
    for r in radii:
        want, on_edge, most = ec.neighbor_sum_exact(cloud, r, cand)
        assert (want[~cloud["side"]] == 0).all() and most >= 2
        if r >= 3.0:
            assert (want != cloud["w"] * cloud["side"]).sum() > n // 4  # the sums are not the atoms' own weights
        if lattice and r in (3.0, 5.0, 13.0):
            assert on_edge >= 1000, (name, r, on_edge)
    if lattice and ec.SQRT5 in radii:
        # thousands of lattice pairs sit at d^2 = 5, 2, 3 (and 13): whether they are in is decided by the f32 product alone, and for sqrt 3
        # and sqrt 13 a product formed in f64 decides the other way
        idx, pairs, d2 = cand
        for r, whole, f64_differs in ((ec.SQRT5, 5, False), (ec.SQRT2, 2, False), (ec.SQRT3, 3, True), (ec.SQRT13, 13, True)):
            if r not in radii:
                continue
            assert (d2 == whole * ec.SCALE ** 2).sum() >= 1000
            in_f32, in_f64 = ec.r_squared(r) >= whole, float(np.float32(r)) * float(np.float32(r)) >= whole
            assert (in_f32 != in_f64) == f64_differs and in_f32 == (whole != 2), r
