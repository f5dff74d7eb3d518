"""Secondary structure (arp_dssp) on its decision thresholds and launch boundaries, without a device: every case of tests/dssp_edge_cases.py through the host twin
arp_dssp_host, which must equal the Python-float restatement there (decisions, acceptors, and hb_energy as one rounding of the restated f64 to f32); the pinned
strings; and the reach checks -- every sweep contains both outcomes, every "exactly on" value is bit-exactly on, the crowded case fills every mask, the six
arrival orders are six different index orders.  tests/test_dssp_edge_gpu.py runs the same cases on the device.  No case is skipped or built again with another
seed; expected values never come from the call under test.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import arpeggia_amd as aa
import dssp_cases as dc
import dssp_edge_cases as ec


def twin(case: dict) -> dict:
    return aa.secondary_structure_host(case["xyz"], case["flags"])


@pytest.mark.parametrize("name", ec.NAMES)
def test_twin_is_the_restatement(name):
    case, want = ec.case(name), ec.want(name)
    got = twin(case)
    for key in ("codes", "counts", "frame_counts", "hb_acceptor"):
        assert np.array_equal(got[key], want[key]), (name, key, np.argwhere(got[key] != want[key])[:5].tolist())
    assert np.array_equal(got["hb_energy"], want["hb_energy"].astype(np.float32)), name      # one rounding of the restated f64
    if "string" in case:
        assert ec.strings(got["codes"]) == [case["string"]] * len(got["codes"]), name


def bonded(name: str, i: int, j: int) -> list:
    return [(i, j) in fr["hb"] for fr in ec.want(name)["frames"]]


# ---- reach checks -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_energy_edge_is_reached():
    """x0 and its successor are adjacent doubles with E < -0.5 and not; the sweep holds both outcomes, each frame's decision is the restated one, and the only
    energy of the input is that of the bond a -> a + 3."""
    xs, x0 = ec.energy_edge()
    x1 = math.nextafter(x0, math.inf)
    assert ec.probe_energy(x0) < -0.5 and not ec.probe_energy(x1) < -0.5 and 5.0 < x0 < 5.3
    assert len(xs) >= 13 and xs[6] == x0 and xs[7] == x1
    want = ec.want("energy")
    flags = bonded("energy", 0, 3)
    assert flags == [ec.probe_energy(x) < -0.5 for x in xs] and True in flags and False in flags
    assert all(set(fr["pairs"]) == {(0, 3)} for fr in want["frames"])
    assert all(abs(fr["pairs"][(0, 3)] + 0.5) < 1e-12 for fr in want["frames"])
    assert ec.strings(want["codes"]) == ["-TT---" if b else "------" for b in flags]
    assert [x for x in xs[13:]] == [x for x in xs[13:] if ec.probe_energy(x) == -0.5]        # (the frames exactly on -0.5, if the scan found any: no bond)
    assert not any(flags[13:])
    # E = -0.5 exactly is no value of the definition: 27.888 S steps over 0.5 between two neighbouring doubles S, so E < -0.5 and E <= -0.5 decide alike on every
    # input, and what can be pinned is the decision at the adjacent doubles either side of the flip
    s0 = 0.5 / 27.888
    around = [ec.ulps(s0, k) for k in range(-8, 9)]
    assert all(27.888 * s != 0.5 for s in around) and 27.888 * around[0] < 0.5 < 27.888 * around[-1] and len(xs) == 13


@pytest.mark.parametrize("name,a", [("ca", 0), ("ca_a62", 62)])
def test_ca_cut_is_reached(name, a):
    """prev(9) gives the pair; 9 exactly, next(9), 9.05 and 9.055 pass the prefilter (d^2 < 82) and fail the cut; 9.06 fails the prefilter."""
    case, want = ec.case(name), ec.want(name)
    ca = case["xyz"][:, :, 1]
    d = [ec.dist(ca[f, a].tolist(), ca[f, a + 3].tolist()) for f in range(len(ec.CA_SWEEP))]
    assert d == list(ec.CA_SWEEP) and d[1] == 9.0 and d[0] < 9.0 < d[2]
    d2 = [float(((ca[f, a] - ca[f, a + 3]) ** 2).sum()) for f in range(len(d))]
    assert [v < ec.FAR2 for v in d2] == [True] * 5 + [False]
    assert bonded(name, a, a + 3) == [True] + [False] * 5
    assert [len(fr["pairs"]) for fr in want["frames"]] == [1, 0, 0, 0, 0, 0]
    assert (want["hb_acceptor"][1:] == ec.NONE).all() and ec.strings(want["codes"][1:]) == ["-" * len(case["res"])] * 5
    assert ec.strings(want["codes"][:1]) == ["-" * a + "-TT-" + "-" * (len(case["res"]) - a - 4)]


def test_break_is_reached():
    case, want = ec.case("break"), ec.want("break")
    x = case["xyz"]
    cn = [ec.dist(x[f, 2, 2].tolist(), x[f, 3, 0].tolist()) for f in range(3)]
    assert cn == list(ec.BREAK_SWEEP) and cn[1] == 2.5 and cn[0] < 2.5 < cn[2]
    assert [fr["brk"][3] for fr in want["frames"]] == [False, False, True]
    assert bonded("break", 0, 3) == [True, True, False]
    assert want["hb_acceptor"][:, 3, 0].tolist() == [0, 0, ec.NONE] and ec.strings(want["codes"]) == ["-TT---", "-TT---", "------"]


def test_minimum_distance_is_reached():
    """Each of the four distances at prev(0.5), 0.5 and next(0.5), the other three above 0.5: the first is clamped to -9.9 exactly, the others give the formula."""
    case, want = ec.case("min"), ec.want("min")
    plan = ec.min_variants()
    assert [(w, v) for w, v, _ in plan] == [(w, v) for v in ec.MIN_SWEEP for w in ec.MIN_WHICH]
    for f, (which, v, _) in enumerate(plan):
        x = case["xyz"][f].tolist()
        h = ec.hydrogen(x[3][0], x[2][2], x[2][3])
        assert h == [1.0, 0.0, 0.0]
        e, d = ec.energy(x[0][3], x[0][2], x[3][0], h)
        k = ec.MIN_WHICH.index(which)
        assert d[k] == v and all(d[m] > 0.6 for m in range(4) if m != k), (which, v, d)
        assert want["frames"][f]["pairs"] == {(0, 3): e}
        assert e == -9.9 if v < 0.5 else abs(e) > 20.0, (which, v, e)          # (at 0.5 the formula gives about -31, +29, -29, -31 here)
        assert want["hb_acceptor"][f, 3].tolist() == [0, ec.NONE]
    assert ec.MIN_SWEEP[1] == 0.5 and ec.MIN_SWEEP[0] < 0.5 < ec.MIN_SWEEP[2]


@pytest.mark.parametrize("name,a", [("bend", 0), ("bend_a254", 254)])
def test_bend_edge_is_reached(name, a):
    ts_, t0 = ec.bend_edge()
    t1 = math.nextafter(t0, math.inf)
    assert not ec.bend_cos(t0) < dc.COS70 and ec.bend_cos(t1) < dc.COS70 and abs(math.degrees(t0) - 70.0) < 1e-9
    want = ec.want(name)
    bends = [ec.bend_cos(t) < dc.COS70 for t in ts_]
    assert True in bends and False in bends
    R = len(ec.case(name)["res"])
    assert ec.strings(want["codes"]) == ["-" * (a + 2) + ("S" if b else "-") + "-" * (R - a - 3) for b in bends]
    assert all(not fr["pairs"] for fr in want["frames"])


@pytest.mark.parametrize("i,j,R", ec.BRIDGE_PLACES)
def test_bridge_sweep_is_reached(i, j, R):
    """The bridge stands iff both bonds stand; the two energies are bit-equal functions of their x, so the two halves of the sweep decide alike."""
    name = f"bridge_{i}_{j}"
    want = ec.want(name)
    xs = ec.energy_edge()[0]
    n = len(xs)
    swept = [ec.probe_energy(x) < -0.5 for x in xs]
    assert bonded(name, i, j) == [True] * n + swept and bonded(name, j, i) == swept + [True] * n
    for f, fr in enumerate(want["frames"]):
        x1, x2 = (3.0, xs[f]) if f < n else (xs[f - n], 3.0)
        assert fr["pairs"] == {(i, j): ec.probe_energy(x1), (j, i): ec.probe_energy(x2)}
    both = swept + swept
    assert True in swept and False in swept
    row = lambda b: "".join("B" if b and r in (i, j) else "-" for r in range(R))
    assert ec.strings(want["codes"]) == [row(b) for b in both]
    assert i // ec.TILE != j // ec.TILE or R == 8


@pytest.mark.parametrize("a", sorted(ec.PLACES))
def test_placements(a):
    name = "energy" if a == 0 else f"place_{a}"
    case, want = ec.case(name), ec.want(name)
    R = len(case["res"])
    assert R == a + 4 + ec.PLACES[a]
    flags = [ec.probe_energy(x) < -0.5 for x in ec.energy_edge()[0]]
    assert bonded(name, a, a + 3) == flags
    assert ec.strings(want["codes"]) == ["-" * a + ("-TT-" if b else "----") + "-" * (R - a - 4) for b in flags]
    assert {len(ec.case("energy" if p == 0 else f"place_{p}")["res"]) for p in ec.PLACES} >= {64, 65, 256, 257}


def test_two_best_plan():
    """The hand-derived entries of every frame equal the restated ones; the six orders are six different index orders; tied energies are bit-equal."""
    want = ec.want("best")
    plan = ec.best_plan()
    orders = set()
    for f, (name, put, entries) in enumerate(plan):
        fr = want["frames"][f]
        assert [i for i, _ in fr["best"][ec.DONOR]] == entries, name
        assert {i for i, _ in fr["pairs"]} == set(put) and {j for _, j in fr["pairs"]} == {ec.DONOR}
        if name.startswith("order"):
            orders.add(tuple(sorted(put, key=lambda s: fr["pairs"][(s, ec.DONOR)])))
            assert len({fr["pairs"][(s, ec.DONOR)] for s in put}) == 3
    assert len(orders) == 6
    assert len({s // ec.TILE for s in (5, 70, 135, ec.DONOR)}) == 4 and 5 // ec.TILE == 6 // ec.TILE
    e = lambda name, s: want["frames"][[p[0] for p in plan].index(name)]["pairs"][(s, ec.DONOR)]
    assert e("tie_same_tile", 5) == e("tie_same_tile", 6) < e("tie_same_tile", 70)
    assert e("tie_across_tiles", 5) == e("tie_across_tiles", 70) < e("tie_across_tiles", 135)
    assert e("tie_for_second_then_better", 135) < e("tie_for_second_then_better", 5) == e("tie_for_second_then_better", 70)
    assert e("tie_for_second_after_better", 5) < e("tie_for_second_after_better", 70) == e("tie_for_second_after_better", 135)
    assert {e("four_clamped", s) for s in ec.SLOTS} == {-9.9} and {e("three_clamped", s) for s in (5, 70, 135)} == {-9.9}


def test_crowded_masks_are_full():
    """Every CA within the cut (and so below the prefilter's bound) of every other: each donor's mask holds every acceptor of every tile but itself and its
    predecessor; the last tile holds two.  The two best also by the numpy restatement of tests/dssp_cases.py."""
    case, want = ec.case("crowded"), ec.want("crowded")
    R = ec.CROWD_R
    assert R == 2 * ec.TILE + 2
    ca = case["xyz"][0, :, 1]
    d2 = ((ca[:, None] - ca[None]) ** 2).sum(-1)
    assert d2.max() < 64.0 < ec.FAR2
    fr = want["frames"][0]
    assert fr["donor"] == [False] + [True] * (R - 1)
    assert len(fr["pairs"]) == (R - 1) * (R - 2)              # every donor j >= 1 against every i but j and j - 1
    g = dc.geometry(case["xyz"][0], case["flags"])
    for j in range(R):
        col = np.where(np.isnan(g["E"][:, j]), np.inf, g["E"][:, j])
        order = np.argsort(col, kind="stable")[:2]
        assert [int(i) if np.isfinite(col[i]) else ec.NONE for i in order] == [i for i, _ in fr["best"][j]], j
    assert sum(1 for e in fr["pairs"].values() if e == -9.9) >= 2          # (clamped pairs exist: ties at -9.9 are decided by the index)


def test_margin_cases_keep_their_margins():
    for name in ec.MARGIN_CASES:
        case = ec.case(name)
        assert dc.clear(case["xyz"], case["flags"]), name
    assert ec.strings(ec.want("split_pro")["codes"]) == [ec.SPLIT_STRING]        # the proline on residue 130 changes nothing
    assert ec.case("split_pro")["flags"][ec.PROLINE_AT] == dc.NO_H and (ec.PROLINE_AT - 4, ec.PROLINE_AT) in ec.want("split")["frames"][0]["hb"]
    assert (ec.PROLINE_AT - 4, ec.PROLINE_AT) not in ec.want("split_pro")["frames"][0]["hb"]
    for k in ec.UBQ_PADS:
        assert np.array_equal(ec.want(f"ubq_pad{k}")["counts"][:, 0] == 3, np.array([c == "-" for c in ec.case(f"ubq_pad{k}")["string"]]))
        helix = range(k + 22, k + 34)
        hairpin = range(k, k + 17)
        assert any(b in r for r in (helix, hairpin) for b in (ec.TILE, ec.ASSIGN)), k     # (k = 64: the chain starts on residue 64, the first of a tile)
