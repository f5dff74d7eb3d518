"""k_neighbor_sum (arpeggia_amd/csrc/sap.inl) bit for bit: on clouds whose coordinates are multiples of 2^-8 and whose weights are multiples
of 1/8 every f64 distance and every f32 partial sum is exact in any order, so the device must equal the int64 reference of
tests/sasa_edge_cases.py exactly -- one dropped, doubled or misjudged neighbour of weight 1/8 shows.  Below and above 196 608 atoms (nine and
three waves per task), radii whose square sits exactly on thousands of lattice distances, the inclusive edge far from the origin."""
from fractions import Fraction

import numpy as np
import pytest

import arpeggia_amd as aa
import sasa_edge_cases as edge

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


@pytest.mark.parametrize("name", [c[0] for c in edge.SUM_CLOUDS])
def test_sums_on_dyadic_clouds_are_exact(ctx, name):
    _, n, lattice, side, radii = edge.SUM_CLOUDS[[c[0] for c in edge.SUM_CLOUDS].index(name)]
    cloud = edge.sum_cloud(name)
    assert (n >= edge.SPLIT3_FROM) == ("230k" in name)
    cand = edge.candidate_pairs(cloud, radii[0])
    for r in radii:
        want, on_edge, most = edge.neighbor_sum_exact(cloud, r, cand)
        got = aa.sap_neighbor_sum(ctx, cloud["x"], cloud["y"], cloud["z"], cloud["side"], cloud["w"], r)
        assert got.dtype == np.float32
        wrong = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        # (-0.0 cannot arise: a sum starts from +0.0f and x + (-x) rounds to +0.0)
        assert len(wrong) == 0, (name, r, len(wrong), wrong[:5].tolist(), got[wrong[:5]].tolist(), want[wrong[:5]].tolist())
        assert (got[~cloud["side"]] == 0).all()


def test_zero_radius_counts_coincident_atoms_only(ctx):
    cloud = edge.sum_cloud("lattice_60k")
    ones = np.ones(len(cloud["x"]), np.float32)
    got = aa.sap_neighbor_sum(ctx, cloud["x"], cloud["y"], cloud["z"], cloud["side"], ones, 0.0)
    sites, inverse, per_site = np.unique(cloud["q"][cloud["side"]], axis=0, return_inverse=True, return_counts=True)
    assert per_site.max() >= 3
    assert np.array_equal(got[cloud["side"]], per_site[inverse.reshape(-1)].astype(np.float32))


def _edge_set(x0: float):
    """Two pairs along x: exactly 5 apart (in: the test is inclusive) and one f64 step more than 5 apart (out)."""
    x = np.array([x0, x0 + 5.0, x0, float(np.nextafter(np.float64(x0 + 5.0), np.inf))])
    y = np.array([0.0, 0.0, 50.0, 50.0])
    assert Fraction(x[1]) - Fraction(x[0]) == 5 and Fraction(x[3]) - Fraction(x[2]) > 5
    dx = x[3] - x[2]
    assert dx * dx > 25.0  # the f64 squared distance of the contract is above r^2 as well
    return x, y, np.zeros(4)


@pytest.mark.parametrize("x0", [0.0, 1.0e4, -1.0e4])
def test_inclusive_edge_far_from_the_origin(ctx, x0):
    x, y, z = _edge_set(x0)
    one, all_sc = np.ones(4, np.float32), np.ones(4, np.uint8)
    assert aa.sap_neighbor_sum(ctx, x, y, z, all_sc, one, 5.0).tolist() == [2.0, 2.0, 1.0, 1.0]


@pytest.mark.parametrize("far", [1.0e4, 1.0e5, 1.0e6])
def test_inclusive_edge_with_a_far_second_cluster(ctx, far):
    """The f32 prefilter margin grows with the box: the decision still falls to the f64 test."""
    x, y, z = _edge_set(0.0)
    x2, y2, z2 = _edge_set(far)
    x, y, z = np.concatenate([x, x2]), np.concatenate([y, y2 + far]), np.concatenate([z, z2 - far])
    w = np.array([1.0, 0.5, 0.25, 0.125, -1.0, -0.5, -0.25, -0.125], np.float32)
    got = aa.sap_neighbor_sum(ctx, x, y, z, np.ones(8, np.uint8), w, 5.0)
    assert got.tolist() == [1.5, 1.5, 0.25, 0.125, -1.5, -1.5, -0.25, -0.125]
