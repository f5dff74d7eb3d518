"""Torsion angles (arp_torsions) on the device, ON their decision thresholds and launch boundaries.

The cases of tests/torsion_edge_cases.py through arp_torsions (as tests/test_torsion_gpu.py calls it): k_torsion_stats past its first chunk of 1024 frames
(blockIdx.y >= 1), with transitions that are read across a chunk boundary and an undefined frame on one, and past 64 torsions (blockIdx.x = 1); the exact angles
180, 0, +-90 and their mirror images at four bin counts; subnormal and signed-zero sines (a device that flushed f64 subnormals would call g- g+); c = -0.5 one
ulp at a time; the 1-degree grid and the wrap at +-180; k_torsion_hist2_match on partial last waves with differing keys and undefined lanes.  The expected
values are the numpy restatement's or pinned (tests/test_torsion_edge_host.py shows that the host twin gives them too); they never come from the call under test,
except where bit-equality between two calls is the property.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import arpeggia_amd as aa
import torsion_cases as tc
import torsion_edge_cases as te
import trajectory_shapes as ts
from test_torsion_gpu import assert_equal, call, same_bytes

pytestmark = pytest.mark.gpu

KNOBS = ("rmsd_chunk_atoms", "torsion_hist2_route")


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, "<f4").view("<u4")


def bits64(a) -> np.ndarray:
    return np.ascontiguousarray(a, "<f8").view("<u8")


def one_quad(ctx, frames: np.ndarray, B: int) -> dict:
    """One torsion on four atoms, frames [F, 4, 3]."""
    s = aa.Structure.from_records(ts.records(tc.four_atoms(frames[0])))
    return call(ctx._h, s, frames, [[0, 1, 2, 3]], B)


def assert_counts(got: dict, r: dict, B: int, what):
    want = tc.over_frames(r, B)
    for key in ("n_defined", "state_counts", "n_transitions", "hist"):
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5].tolist())
    F = r["state"].shape[0]
    bound = F * 2.0 ** -52 * want["n_defined"].astype(np.float64)[:, None]      # the bound of test_torsion_gpu.assert_equal
    assert (np.abs(got["sums"] - want["sums"]) <= bound).all(), (what, "sums", float(np.abs(got["sums"] - want["sums"]).max()))


@pytest.mark.parametrize("name", sorted(te.STATS))
def test_statistics_chunks(ctx, name):
    """F = 1024, 1025 and 2049 frames: one full chunk, a second chunk of one frame, three chunks; D = 65: a second block of torsions.  The counts and the
    transitions from the restatement, exact; the same bytes when the frames come in passes of 1000 (a pass boundary that is not a chunk boundary)."""
    F, D, hole = te.STATS[name]
    c = te.stats_case(F, D, hole)
    s = aa.Structure.from_records(ts.records(te.atoms_of(c["quads_xyz"][0])))
    r = tc.restate(c["quads_xyz"], 36)
    got = call(ctx._h, s, c["frames"], c["quads"], 36)
    assert np.array_equal(got["states"], c["states"])
    assert_counts(got, r, 36, name)
    aa.debug_set("rmsd_chunk_atoms", 1000 * 4 * D)
    same_bytes(call(ctx._h, s, c["frames"], c["quads"], 36), got, name)


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("B", te.EXACT_BINS)
def test_exact_angles(ctx, B, mirrored):
    got, pin = one_quad(ctx, te.exact_frames(mirrored), B), te.exact_pinned(mirrored, B)
    assert got["angles"][:, 0].tolist() == pin["angles"] and got["states"][:, 0].tolist() == pin["states"] and got["cossin"][:, 0].tolist() == pin["cossin"]
    want = np.zeros(B, np.uint32)
    np.add.at(want, pin["bins"], 1)
    assert np.array_equal(got["hist"][0], want)


def test_sign_of_the_sine(ctx):
    frames = te.sine_frames()
    r = tc.restate(frames[:, None], 36)
    got = one_quad(ctx, frames, 36)
    n = len(te.TINY)
    assert got["states"][:, 0].tolist() == [3 if v < 0 else 1 for v in te.TINY] + [2] * n == r["state"][:, 0].tolist()
    assert np.array_equal(bits64(got["cossin"][:, 0, 0]), bits64(r["c"][:, 0])) and np.array_equal(bits64(got["cossin"][:, 0, 1]), bits64(r["s"][:, 0]))
    want_angle = [-0.0 if v < 0 else 0.0 for v in te.TINY] + [-180.0 if v < 0 else 180.0 for v in te.TINY]      # the twin's bits (test_torsion_edge_host.py)
    assert np.array_equal(bits(got["angles"][:, 0]), bits(np.array(want_angle)))
    assert_counts(got, r, 36, "sine")
    assert got["hist"][0, 18] == n and got["hist"][0, 0] == n


def test_cosine_threshold(ctx):
    frames = te.cosine_frames()
    r = tc.restate(frames[:, None])
    twin = aa.torsions_host(frames[:, None])
    got = one_quad(ctx, frames, 36)
    assert np.array_equal(bits64(got["cossin"]), bits64(twin["cossin"]))
    assert got["states"][:, 0].tolist() == [2 if c <= -0.5 else 1 for c in r["c"][:, 0].tolist()]
    assert set(got["states"][:, 0].tolist()) == {1, 2} and -0.5 in r["c"][:, 0].tolist()


def test_grid(ctx):
    frames = te.grid_frames(0.0)
    r = tc.restate(frames[:, None], 360)
    got = one_quad(ctx, frames, 360)
    assert np.abs(got["angles"][:, 0].astype(np.float64) - te.GRID).max() <= 2e-5
    assert np.array_equal(got["states"], r["state"]) and np.array_equal(bits64(got["cossin"]), bits64(np.stack([r["c"], r["s"]], -1)))
    frames = te.grid_frames(0.5)
    r = tc.restate(frames[:, None], 360)
    got = one_quad(ctx, frames, 360)
    assert got["hist"][0].tolist() == [0] + [1] * 359
    assert_counts(got, r, 360, "shifted grid")


@lru_cache(maxsize=None)
def ubq():
    s = aa.Structure.load(str(tc.DATA / "1ubq.pdb"))
    soa = s.soa()
    return s, aa.torsion_select(s), np.stack([soa["x"], soa["y"], soa["z"]], 1).astype(np.float64)


@pytest.mark.parametrize("F", te.MATCH_FRAMES)
def test_wave_matched_maps(ctx, F):
    """The class groups with the matched route forced, against the restatement and the twin; the three routes: the same bytes; one group per residue (76 x 36 x 36
    words do not fit the LDS tables: the matched route by itself)."""
    s, sel, xyz = ubq()
    c = te.matched_case(xyz, sel["quads"], F, sel["quads"][sel["pairs"][0, 1]][:3])
    q = tc.gather(c["frames"], c["quads"])
    r = tc.restate(q, 36)
    aa.debug_set("torsion_hist2_route", 2)
    matched = call(ctx._h, s, c["frames"], c["quads"], 36, sel["pairs"], 4)
    assert np.array_equal(matched["hist2"], tc.over_frames(r, 36, sel["pairs"], 4)["hist2"])
    assert_equal(matched, aa.torsions_host(q, sel["pairs"], 4, 36), F)
    for route in (1, 3):
        aa.debug_set("torsion_hist2_route", route)
        same_bytes(call(ctx._h, s, c["frames"], c["quads"], 36, sel["pairs"], 4), matched, route)
    aa.debug_set("torsion_hist2_route", 0)
    R = sel["n_rows"]
    assert R * 36 * 36 * 4 > tc.LDS_BYTES
    per_res = sel["pairs"].copy()
    per_res[:, 2] = sel["row"][sel["pairs"][:, 0]]
    got = call(ctx._h, s, c["frames"], c["quads"], 36, per_res, R)
    assert np.array_equal(got["hist2"], tc.over_frames(r, 36, per_res, R)["hist2"])
    assert len(tc.SKIPPED_SEEDS) <= 1


@pytest.mark.parametrize("route", [2, 1, 3])
def test_inactive_lanes_are_not_counted(ctx, route):
    """The pair's key is 0 (bin (0, 0)) in most frames, which is also what a lane without a sample carries: torsion 0 is undefined in frame 3, and in frame 65
    of a second wave that holds frame 64 (key 0) and 62 lanes past the frames.  Bin (0, 0) holds the defined samples and nothing else."""
    c = te.key_zero_case()
    s = aa.Structure.from_records(ts.records(te.atoms_of(c["quads_xyz"][0])))
    want = tc.over_frames(tc.restate(c["quads_xyz"], 36), 36, c["pairs"], 1)
    aa.debug_set("torsion_hist2_route", route)
    got = call(ctx._h, s, c["frames"], c["quads"], 36, c["pairs"], 1)
    assert np.array_equal(got["hist2"], want["hist2"]) and np.array_equal(got["hist"], want["hist"])
    assert int(got["hist2"][0, 0, 0]) == te.KEY_ZERO_FRAMES - 2 - len(range(2, te.KEY_ZERO_FRAMES, 5)) and int(got["hist2"].sum()) == te.KEY_ZERO_FRAMES - 2
