"""Torsion angles (arp_torsions) on their decision thresholds and launch boundaries, without a device: every case of tests/torsion_edge_cases.py through the host
twin arp_torsions_host against the numpy restatement of tests/torsion_cases.py and the values pinned there, and the reach checks -- the sweeps contain both
outcomes, the chunk boundaries carry the transitions they are built for.  tests/test_torsion_edge_gpu.py runs the same cases on the device.  Expected values
never come from the call under test.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import arpeggia_amd as aa
import torsion_cases as tc
import torsion_edge_cases as te


def twin(q, B=36, pairs=None, G=0):
    return aa.torsions_host(q, pairs, G, B)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, "<f4").view("<u4")


def bits64(a) -> np.ndarray:
    return np.ascontiguousarray(a, "<f8").view("<u8")


def assert_counts(res: dict, r: dict, B: int, pairs=None, G=0):
    want = tc.over_frames(r, B, pairs, G)
    for key in ("n_defined", "state_counts", "n_transitions", "hist") + (("hist2",) if G else ()):
        assert np.array_equal(res[key], want[key]), key
    F = r["state"].shape[0]
    assert (np.abs(res["sums"] - want["sums"]) <= F * 2.0 ** -52 * np.maximum(want["n_defined"], 1)[:, None]).all()


@pytest.mark.parametrize("name", sorted(te.STATS))
def test_statistics_chunks(name):
    F, D, hole = te.STATS[name]
    c = te.stats_case(F, D, hole)
    r = tc.restate(c["quads_xyz"], 36)
    assert np.array_equal(r["state"], c["states"])         # the frames are in the states they were built for
    res = twin(c["quads_xyz"])
    assert np.array_equal(res["states"], c["states"])
    assert_counts(res, r, 36)
    # reach: the boundary transitions are there and counted, the hole is not
    st = c["states"]
    for f in (te.STATS_FRAMES, 2 * te.STATS_FRAMES):
        if f < F:
            edge = st[f - 1, 0] == 1 and st[f, 0] == 2
            assert edge
    if hole:
        assert st[1023:1026, D - 1].tolist() == [1, 0, 2]
    assert set(np.unique(st).tolist()) == {0, 1, 2, 3} and res["n_transitions"].min() > F // 4
    if D > te.WAVE:
        assert len({st[:, d].tobytes() for d in range(D)}) == D      # independent sequences


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("B", te.EXACT_BINS)
def test_exact_angles(B, mirrored):
    q = te.exact_frames(mirrored)[None]
    res, pin = twin(q, B), te.exact_pinned(mirrored, B)
    assert res["angles"][0].tolist() == pin["angles"] and res["states"][0].tolist() == pin["states"] and res["cossin"][0].tolist() == pin["cossin"]
    assert [np.flatnonzero(row).tolist() for row in res["hist"]] == [[b] for b in pin["bins"]]
    r = tc.restate(q, B)
    assert r["a"][0].tolist() == pin["angles"] and r["bin"][0].tolist() == pin["bins"]     # numpy gives the same special cases


def test_sign_of_the_sine():
    q = te.sine_frames()[None]
    r = tc.restate(q, 36)
    res = twin(q, 36)
    n = len(te.TINY)
    assert r["c"][0].tolist() == [1.0] * n + [-1.0] * n
    assert np.array_equal(bits64(r["s"][0]), bits64(np.array([v + 0.0 if v == 0 else v for v in te.TINY] * 2)))      # (y = v + 0 u: -0 becomes +0)
    assert np.array_equal(res["states"], r["state"]) and np.array_equal(bits64(res["cossin"][..., 0]), bits64(r["c"])) and np.array_equal(bits64(res["cossin"][..., 1]), bits64(r["s"]))
    want_state = [3 if v < 0 else 1 for v in te.TINY] + [2] * n        # negative subnormal sines are g-; c = -1 is t whatever the sine
    assert res["states"][0].tolist() == want_state
    assert np.array_equal(np.argmax(res["hist"], 1), r["bin"][0]) and (res["hist"].sum(1) == 1).all()
    assert r["bin"][0].tolist() == [18] * n + [0] * n                   # +-0 in bin 18; +180 wraps to bin 0, where -180 is
    want_angle = [-0.0 if v < 0 else 0.0 for v in te.TINY] + [-180.0 if v < 0 else 180.0 for v in te.TINY]
    assert np.array_equal(bits(res["angles"][0]), bits(np.array(want_angle)))
    assert np.array_equal(bits(res["angles"]), bits(r["a"].astype(np.float32)))


def test_cosine_threshold():
    q = te.cosine_frames()[None]
    r = tc.restate(q)
    res = twin(q)
    assert np.array_equal(bits64(res["cossin"][..., 0]), bits64(r["c"])) and np.array_equal(bits64(res["cossin"][..., 1]), bits64(r["s"]))
    assert np.array_equal(res["states"], r["state"])
    assert res["states"][0].tolist() == [2 if c <= -0.5 else 1 for c in r["c"][0].tolist()]
    assert set(res["states"][0].tolist()) == {1, 2} and -0.5 in r["c"][0].tolist()
    assert (np.diff(r["c"][0]) >= 0).all()


def test_grid():
    q = te.grid_frames(0.0)[:, None]
    res, r = twin(q, 360), tc.restate(q, 360)
    assert np.abs(res["angles"][:, 0].astype(np.float64) - te.GRID).max() <= 2e-5
    assert np.array_equal(res["states"], r["state"]) and np.array_equal(bits64(res["cossin"]), bits64(np.stack([r["c"], r["s"]], -1)))
    q = te.grid_frames(0.5)[:, None]
    res, r = twin(q, 360), tc.restate(q, 360)
    assert tc.edge_margin(r["a"], 360) > 0.49
    assert r["bin"][:, 0].tolist() == (te.GRID[:-1] + 180).tolist()
    assert res["hist"][0].tolist() == [0] + [1] * 359
    assert_counts(res, r, 360)


@lru_cache(maxsize=None)
def ubq():
    s = aa.Structure.load(str(tc.DATA / "1ubq.pdb"))
    soa = s.soa()
    return s, aa.torsion_select(s), np.stack([soa["x"], soa["y"], soa["z"]], 1).astype(np.float64)


@pytest.mark.parametrize("F", te.MATCH_FRAMES)
def test_matched_cases(F):
    _, sel, xyz = ubq()
    line = sel["quads"][sel["pairs"][0, 1]][:3]                      # N, CA, C of the first residue that has a (phi, psi) pair: its psi
    c = te.matched_case(xyz, sel["quads"], F, line)
    q = tc.gather(c["frames"], c["quads"])
    r = tc.restate(q, 36)
    through = np.flatnonzero(np.isin(sel["quads"][:, :3], line).all(1) | np.isin(sel["quads"][:, 1:], line).all(1))        # three consecutive atoms on the line
    assert len(through) >= 1 and not r["defined"][list(c["collinear"])][:, through].any() and r["defined"][0].all()
    per_res = sel["pairs"].copy()
    per_res[:, 2] = sel["row"][sel["pairs"][:, 0]]
    for pairs, G in ((sel["pairs"], 4), (per_res, sel["n_rows"])):
        res = twin(q, 36, pairs, G)
        assert np.array_equal(res["states"], r["state"])
        assert_counts(res, r, 36, pairs, G)
    hit = np.isin(sel["pairs"][:, :2], through).any(1)
    assert hit.any() and int(res["hist2"].sum()) == F * len(sel["pairs"]) - 2 * int(hit.sum())        # lanes do drop out
    assert len(tc.SKIPPED_SEEDS) <= 1


def test_key_zero_case():
    c = te.key_zero_case()
    F = te.KEY_ZERO_FRAMES
    r = tc.restate(c["quads_xyz"], 36)
    res = twin(c["quads_xyz"], 36, c["pairs"], 1)
    assert_counts(res, r, 36, c["pairs"], 1)
    assert F % te.WAVE == 2 and c["undefined"] == (3, F - 1) and np.flatnonzero(~r["defined"][:, 0]).tolist() == [3, F - 1] and r["defined"][:, 1].all()
    other = sum(1 for f in range(F) if f % 5 == 2 and f not in c["undefined"])
    assert other == len(range(2, F, 5)) and r["bin"][64].tolist() == [0, 0]
    assert int(res["hist2"][0, 0, 0]) == F - 2 - other and int(res["hist2"][0, 0, 24]) == other and int(res["hist2"].sum()) == F - 2
