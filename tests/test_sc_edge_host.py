"""The cases of tests/sc_edge_cases.py through the sequential restatement (tests/sc_restatement.c) alone, on the CPU: every case reaches
the path it is named for (the restatement's reach counters, sc_restatement.REACH), and the facts that do not need a device -- the sphere's
area, the strict and the inclusive side of sep, the far atom that changes nothing -- hold for the reference side of tests/test_sc_edge_gpu.py.

Restatement wall time per case on one core of the authoring machine (cc -O2), with the total dot count:
    lat_chunks_contact   density 1.3 s (70 266 dots; latitudes up to 140)   radii 0.65 s (58 904; up to 128)
    lat_chunks_concave   rp3.5_d180 / d190 / d200  0.16 / 0.18 / 0.17 s (61 202 / 64 663 / 68 150; probe latitudes 64 / 66 / 68)
    two_big_spheres      0.03 s (13 564)
    sep_binding          sep5.0 1.6 s (33 033)   sep6.5 1.9 s (38 183)   r2.5 0.18 s (15 965)
    sep_edge             < 0.01 s each
    burial_beyond_sep    < 0.01 s (1 367)
    wide_box             none 2.2 s   three_level 2.0 s   capped 1.7 s (40 628 each)
    settings_sweep       band0.2 1.2 s (450 atoms)   band3.0 1.6 s   w2.0 2.1 s   rp0.5 1.6 s (59 793)   rp3.0 1.7 s   combined 1.9 s (300 atoms)
    d2_ties              0.04 s per ordering (9 945)
The cost is in the trim and nearest-neighbour scans, quadratic in the buried dots of the interface, not in the total: the latitude cases
have many dots on few atoms and a small interface.

Concave latitudes: the arc of a probe runs from one of its atoms to its south pole and is at most pi / 2 long.  On concave_inputs() (probes
0.9 A above the plane of their atoms) the largest emitting probe has 64 latitudes at rp = 3.5, density = 180 -- one full chunk -- and 66 at
density = 190, the smallest of the scanned points (rp 3.0 / 3.5 / 4.0, density 120 .. 220 in steps of 10) past 64; rp = 3.0 reaches 59 and
rp = 4.0 reaches 66 only at density = 220."""
from __future__ import annotations

import numpy as np
import pytest

import sc_edge_cases as E
import sc_restatement as R


@pytest.fixture(scope="module")
def scr(tmp_path_factory):
    return R.compile(tmp_path_factory.mktemp("scr"))


_RUNS = {}


def run(scr, key, case):
    """The restatement's result for a case, computed once per module and left unchanged."""
    if key not in _RUNS:
        inp, st = case
        _RUNS[key] = R.run(scr, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"], inp.get("serial"), **st)
    return _RUNS[key]


def default_run(scr, n_atoms):
    return run(scr, ("halves", n_atoms), (E.halves(n_atoms), dict(E.DEFAULTS)))


def test_counters_are_zero_at_the_defaults(scr):
    # what the existing parity inputs look like: one chunk of latitudes, no tie, sep never binding
    rc = default_run(scr, 600)["reach"]
    assert 0 < rc["max_lat_contact"] <= 24 and 0 < rc["max_lat_probe"] <= 20
    assert rc["d2_ties"] == 0 and rc["kmap_rejects"] == 0 and rc["sep_rejects"] == 0


@pytest.mark.parametrize("name", list(E.lat_chunks_contact()))
def test_lat_chunks_contact_reach(scr, name):
    inp, st = case = E.lat_chunks_contact()[name]
    out = run(scr, ("contact", name), case)
    assert out["err"] == 0 and out["n_convex"] > 0
    # atoms below one chunk (their whole meridian has fewer than 64 samples) next to atoms past it
    assert np.pi * inp["r"].min() * np.sqrt(st["density"]) < 64 < np.pi * inp["r"].max() * np.sqrt(st["density"])
    top = out["reach"]["max_lat_contact"]
    if name == "density":
        assert top > 128, top  # three chunks (measured: 140)
    else:
        assert top == 128, top  # two chunks, both full: the loop's `c0 < nl` ends on the boundary itself


@pytest.mark.parametrize("name", list(E.lat_chunks_concave()))
def test_lat_chunks_concave_reach(scr, name):
    case = E.lat_chunks_concave()[name]
    out = run(scr, ("concave", name), case)
    assert out["err"] == 0 and out["n_concave"] > 0
    top = out["reach"]["max_lat_probe"]
    if case[1]["density"] == 180.0:
        assert top == 64, top  # exactly one full chunk
    else:
        assert top > 64, top  # (measured: 66 at density 190, 68 at 200)
        # and the latitudes of the second chunk emit: without atom 7 over the triangle the probe's mirror image across the plane of its
        # atoms is a near of it and cuts every dot around the south pole, where those latitudes lie (measured: 15 and 47 dots)
        assert out["reach"]["probe_dots_past_64"] > 0


def test_two_big_spheres(scr):
    inp, st = case = E.two_big_spheres()
    out = run(scr, "two_big_spheres", case)
    assert out["err"] == 0 and out["reach"]["max_lat_contact"] == 73
    a0, a1 = (out["dots"][s]["area"] for s in range(2))
    assert len(a0) == len(a1) == 6782 and out["n_convex"] == 2 * 6782 and out["n_toroidal"] == out["n_concave"] == 0
    # the restatement's own deviation from 4 pi r^2 is +1.32e-4 relative (measured: 452.449 against 452.389); a lost latitude costs about
    # 1 / 73 = 1.4e-2, a lost dot of the 6782 equal-weight ones 1.5e-4
    for a in (a0, a1):
        assert abs(a.sum() / (4.0 * np.pi * 36.0) - 1.0) < E.SPHERE_AREA_RTOL


@pytest.mark.parametrize("name", list(E.sep_binding()))
def test_sep_binding_reach(scr, name):
    inp, st = case = E.sep_binding()[name]
    out = run(scr, ("sep", name), case)
    assert out["err"] == 0
    assert out["reach"]["sep_rejects"] > 0 and out["reach"]["kmap_rejects"] > 0, out["reach"]
    if name == "r2.5":  # the atoms' cell edge max(sep, 2 (r_max + rp) + margin) takes its second argument
        assert 2.0 * (inp["r"].max() + st["rp"]) + 0.01 > st["sep"]
    else:  # the bound changes outputs
        base = default_run(scr, 600)
        assert out["n_probes"] < base["n_probes"] and out["n_far_atoms"][0] > base["n_far_atoms"][0]


def test_burial_beyond_sep(scr):
    inp, st = case = E.burial_beyond_sep()
    out = run(scr, "burial_beyond_sep", case)
    assert out["err"] == 0 and out["n_far_atoms"] == [0, 1] and 2.0 * (inp["r"].max() + st["rp"]) > 2.0 * st["sep"]  # two cells of edge sep
    d = out["dots"][0]
    X = np.stack([inp["x"], inp["y"], inp["z"]], 1)
    pcen = X[0] + (d["xyz"] - X[0]) * ((inp["r"][0] + st["rp"]) / inp["r"][0])  # the probe centre of each of atom 0's contact dots
    near1 = ((pcen - X[1]) ** 2).sum(1) <= (inp["r"][1] + st["rp"]) ** 2
    near2 = ((pcen - X[2]) ** 2).sum(1) <= (inp["r"][2] + st["rp"]) ** 2
    buried = (d["flags"] & 4) != 0
    assert np.array_equal(buried, near1 | near2)
    assert (near2 & ~near1).sum() > 0  # dots that only the atom beyond sep buries (measured: 60 of 1179)


def test_sep_edge_outcomes(scr):
    c = E.sep_edge()
    at, inside = run(scr, ("edge", "other_at"), c["other_at"]), run(scr, ("edge", "other_inside"), c["other_inside"])
    assert R.ERRORS[at["err"]] == "No molecular dots generated" and at["n_far_atoms"] == [1, 1]  # d^2 < sep^2 is strict
    assert inside["err"] == 0 and inside["n_buried_atoms"] == [1, 1] and min(inside["n_all_dots"]) > 0
    same, out = run(scr, ("edge", "same_at"), c["same_at"]), run(scr, ("edge", "same_outside"), c["same_outside"])
    assert same["err"] == 0 and same["n_toroidal"] > 0  # d^2 <= sep^2 is inclusive
    assert out["err"] == 0 and out["n_toroidal"] == 0 and out["reach"]["sep_rejects"] == 2  # (the pair, from both sides)


def test_wide_box_cell_counts():
    inp, st = E.wide_box("three_level")
    for edge in (E.TRIM_EDGE, E.open_edge(st)):
        dims, capped = E.cell_dims(inp, st, edge)
        assert not capped and dims[0] * dims[1] * dims[2] + 1 > 1024 * 1024  # the scan of the counts needs a third level
    inp, st = E.wide_box("capped")
    for edge in (E.TRIM_EDGE, E.open_edge(st)):
        dims, capped = E.cell_dims(inp, st, edge)
        # the longest axis (y) has ext / edge = 128, so (int)(ext / edge) + 1 is 129 there; x and z, 0.03 A shorter, have 128: the cap
        # allows 129 cells on an axis, not 128, and cell_of clamps to n - 1
        assert capped and dims == (128, 129, 128), dims
    dims, capped = E.cell_dims(*E.wide_box(None), E.TRIM_EDGE)
    assert not capped and dims[0] * dims[1] * dims[2] < 1024 * 1024  # (the parity inputs stay at two levels)


@pytest.mark.parametrize("which", list(E.WIDE_FAR))
def test_wide_box_far_atom_changes_no_dot(scr, which):
    base, far = default_run(scr, 600), run(scr, ("wide", which), E.wide_box(which))
    assert far["err"] == 0 and far["n_far_atoms"][0] == base["n_far_atoms"][0] + 1
    for k in ("n_convex", "n_toroidal", "n_concave", "n_probes", "sc", "distance", "area"):
        assert far[k] == base[k], k
    for s in range(2):
        for k, v in base["dots"][s].items():
            assert np.array_equal(far["dots"][s][k], v), (s, k)


@pytest.mark.parametrize("name", list(E.settings_sweep()))
def test_settings_sweep_changes_the_result(scr, name):
    inp, st = case = E.settings_sweep()[name]
    out, base = run(scr, ("sweep", name), case), default_run(scr, len(inp["x"]))
    assert out["err"] == 0
    assert out["sc"] != base["sc"] and (out["n_trimmed_dots"] != base["n_trimmed_dots"] or name == "w2.0")
    if name.startswith(("band", "w")):  # the surfaces themselves do not depend on band and w
        assert out["n_all_dots"] == base["n_all_dots"]


def test_d2_ties_reach(scr):
    for seed in E.TIE_ORDERS:
        inp, st = case = E.d2_ties(seed)
        out = run(scr, ("ties", seed), case)
        assert out["err"] == 0 and out["reach"]["d2_ties"] >= 50, out["reach"]
        # ties at the head of a list: neighbour 0 (the contact stage's north pole) is decided by the index
        X = np.stack([inp["x"], inp["y"], inp["z"]], 1)
        heads = 0
        for i in range(len(X)):
            d2 = np.sort(((X - X[i]) ** 2).sum(1)[(inp["mol"] == inp["mol"][i]) & (np.arange(len(X)) != i)])
            heads += int(d2[0] == d2[1])
        assert heads >= 10, heads
    # the order of the atoms decides the ties, so it changes dots (not only their order)
    assert _RUNS[("ties", E.TIE_ORDERS[0])]["n_convex"] != _RUNS[("ties", E.TIE_ORDERS[1])]["n_convex"]
