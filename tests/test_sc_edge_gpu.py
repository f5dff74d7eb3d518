"""Shape complementarity on the device off its default settings and past one wave of latitudes: the cases of tests/sc_edge_cases.py (each
shown by tests/test_sc_edge_host.py to reach the path it is named for) against the sequential restatement, dot for dot, with the
settings of the case passed to both sides.

The comparison is compare() of tests/test_sc_gpu.py, unchanged: counts, kinds and flags equal and in order; positions, normals, areas,
nn_dist and scores within 1e-9 relative; sc, distance and area within 1e-12.  On top of it:
    lat_chunks_*      the counts of the count pass (n_convex, n_concave) equal the restatement's and the kinds the fill pass wrote
    two_big_spheres   the device's dot areas sum to 4 pi r^2 per atom within the host test's bound
    burial_beyond_sep an atom buries dots from farther away than sep: the second argument of the atoms' cell edge (parity alone)
    sep_edge          the error at d = sep between the molecules; toroidal dots at d = sep inside a molecule, none one step outside
    wide_box          the device's dots with the far atom equal the device's dots without it in every field, bit for bit, with more than
                      1024^2 cells (three scan levels) and under the 128-per-axis cap -- a check the restatement is no party to
    d2_ties           three orderings of the atoms, three runs of each: the runs of one ordering are bit-identical.  Across orderings the
                      dots differ by right -- equal d^2 are ordered by atom index, not by serial (tests/test_sc_edge_host.py shows it on
                      the restatement) -- so each ordering is compared with the restatement of the same ordering; what an ordering
                      changes on the device is which lane and which cell rank an atom gets
As in tests/test_sc_gpu.py the device's sin / cos / atan2 / acos / exp differ from glibc's by a few ulps; a case that differed only in a
discrete decision within a few ulps of its bound is to have its input moved, not its assertion relaxed.

Most of a test's time is the restatement (tests/test_sc_edge_host.py lists it per case).  The largest device job, lat_chunks_contact
"density", has 70 266 dots, more than the 25 000 - 40 000 the cases were first sized for: latitudes past 128 need r sqrt(density) above
41, and the dots grow with r^2 density.  It stays within the time limit (1.3 s in the restatement) because the limit is set by the buried
dots of the interface, which is small here (4 267 trimmed dots), not by the total."""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import sc_edge_cases as E
import sc_restatement as R
from test_sc_gpu import compare

pytestmark = pytest.mark.gpu
FIELDS = ("xyz", "normal", "area", "flags", "nn_dist", "score")


@pytest.fixture(scope="module")
def scr(tmp_path_factory):
    return R.compile(tmp_path_factory.mktemp("scr"))


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


def device(ctx, case):
    inp, st = case
    return aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"], inp.get("serial"), E.api_settings(st))


def restated(scr, case):
    inp, st = case
    return R.run(scr, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"], inp.get("serial"), **st)


def parity(ctx, scr, case):
    want = restated(scr, case)
    assert want["err"] == 0
    got = device(ctx, case)
    compare(ctx, want, got)
    return want, got


def kinds(ctx):
    """How many dots of each kind the fill passes wrote (convex, toroidal, concave)."""
    k = np.concatenate([aa.sc_dots(ctx, s)["flags"] & 3 for s in range(2)])
    return [int((k == v).sum()) for v in range(3)]


@pytest.mark.parametrize("name", list(E.lat_chunks_contact()))
def test_lat_chunks_contact(ctx, scr, name):
    want, got = parity(ctx, scr, E.lat_chunks_contact()[name])
    assert got["n_convex"] == want["n_convex"] and got["n_concave"] == want["n_concave"]
    assert kinds(ctx) == [want["n_convex"], want["n_toroidal"], want["n_concave"]]


@pytest.mark.parametrize("name", list(E.lat_chunks_concave()))
def test_lat_chunks_concave(ctx, scr, name):
    want, got = parity(ctx, scr, E.lat_chunks_concave()[name])
    assert got["n_convex"] == want["n_convex"] and got["n_concave"] == want["n_concave"]
    assert kinds(ctx) == [want["n_convex"], want["n_toroidal"], want["n_concave"]]


def test_two_big_spheres(ctx, scr):
    parity(ctx, scr, E.two_big_spheres())
    for s in range(2):
        a = aa.sc_dots(ctx, s)["area"]
        assert len(a) == 6782
        assert abs(a.sum() / (4.0 * np.pi * 36.0) - 1.0) < E.SPHERE_AREA_RTOL


@pytest.mark.parametrize("name", list(E.sep_binding()))
def test_sep_binding(ctx, scr, name):
    parity(ctx, scr, E.sep_binding()[name])


def test_burial_beyond_sep(ctx, scr):
    parity(ctx, scr, E.burial_beyond_sep())


def test_sep_edge(ctx, scr):
    c = E.sep_edge()
    assert R.ERRORS[restated(scr, c["other_at"])["err"]] == "No molecular dots generated"
    with pytest.raises(aa.ArpeggiaError, match="No molecular dots generated"):
        device(ctx, c["other_at"])
    parity(ctx, scr, c["other_inside"])
    _, got = parity(ctx, scr, c["same_at"])
    assert got["n_toroidal"] > 0
    _, got = parity(ctx, scr, c["same_outside"])
    assert got["n_toroidal"] == 0


def device_dots(ctx, case):
    res = device(ctx, case)
    return res, [aa.sc_dots(ctx, s) for s in range(2)]


@pytest.fixture(scope="module")
def near_box(ctx):
    return device_dots(ctx, E.wide_box(None))


@pytest.mark.parametrize("which", list(E.WIDE_FAR))
def test_wide_box(ctx, scr, near_box, which):
    case = E.wide_box(which)
    parity(ctx, scr, case)
    res, dots = device_dots(ctx, case)
    base_res, base_dots = near_box
    for k in ("n_convex", "n_toroidal", "n_concave", "n_probes", "sc", "distance", "area"):
        assert res[k] == base_res[k], k
    for s in range(2):
        for k in FIELDS:
            assert np.array_equal(dots[s][k], base_dots[s][k]), (s, k)


@pytest.mark.parametrize("name", list(E.settings_sweep()))
def test_settings_sweep(ctx, scr, name):
    parity(ctx, scr, E.settings_sweep()[name])


@pytest.mark.parametrize("order", E.TIE_ORDERS)
def test_d2_ties(ctx, scr, order):
    case = E.d2_ties(order)
    parity(ctx, scr, case)
    runs = [device_dots(ctx, case) for _ in range(3)]
    for res, dots in runs[1:]:
        assert res == runs[0][0]
        for s in range(2):
            for k in FIELDS:
                assert np.array_equal(dots[s][k], runs[0][1][s][k]), (s, k)
