"""Cases on the decision thresholds and the launch boundaries of the torsion call (arp_torsions: torsion.inl, one torsion in table_dev.h), built from the pieces
of tests/torsion_cases.py.  No product imports: tests/test_torsion_edge_host.py runs them through the host twin on the CPU, tests/test_torsion_edge_gpu.py
through the device call.  Expected values come from torsion_cases.restate / over_frames or are pinned here.

Launch constants (torsion.inl): k_torsion_stats takes the frames in chunks of STATS_FRAMES = 1024 over blockIdx.y and 64 torsions per blockIdx.x;
k_torsion_hist2_match gives a wave 64 frames of one pair.
"""
from __future__ import annotations

import math

import numpy as np

import torsion_cases as tc
import trajectory_shapes as ts

STATS_FRAMES, WAVE = 1024, 64


# ---- 1: the chunks of the statistics ----------------------------------------------------------------------------------------------------------------------------------
def state_sequence(F: int, seed: int, forced: dict) -> list:
    """A seeded sequence over {0, 1, 2, 3}, with the states of `forced` {frame: state} put over it."""
    seq = np.random.default_rng(seed).integers(0, 4, F).tolist()
    for f, s in forced.items():
        if f < F:
            seq[f] = s
    return seq


CHUNK_EDGE = {STATS_FRAMES - 1: 1, STATS_FRAMES: 2, 2 * STATS_FRAMES - 1: 1, 2 * STATS_FRAMES: 2}      # 1 -> 2 across 1023|1024 and 2047|2048
CHUNK_HOLE = {STATS_FRAMES - 1: 1, STATS_FRAMES: 0, STATS_FRAMES + 1: 2}                                # 1, undefined, 2: no transition


def stats_case(F: int, D: int, hole: bool = False) -> dict:
    """{"states": [F, D] as built, "quads_xyz": [F, D, 4, 3], "frames": [F, 4 D, 3], "quads": [D, 4]}: torsion d on the atoms 4 d .. 4 d + 3, its sequence seeded
    with d; every torsion crosses the chunk boundaries 1 -> 2, except the last one where `hole`, which has frame 1024 undefined between 1 and 2."""
    seqs = [state_sequence(F, 7 + d, CHUNK_HOLE if hole and d == D - 1 else CHUNK_EDGE) for d in range(D)]
    q = np.stack([tc.state_frames(seq) for seq in seqs], 1)
    frames = np.ascontiguousarray(q.reshape(F, 4 * D, 3))
    frames.setflags(write=False)
    return {"states": np.array(seqs, "u1").T, "quads_xyz": q, "frames": frames, "quads": np.arange(4 * D, dtype="<u4").reshape(D, 4)}


STATS = {"F1024": (1024, 1, False), "F1025": (1025, 1, False), "F2049": (2049, 1, False), "F2049_hole": (2049, 2, True), "F1025_D65": (1025, 65, False)}


def atoms_of(quads_xyz: np.ndarray) -> list:
    """Topology atoms (trajectory_shapes.records) of D residues whose N, CA, C, O sit on the D quads of one frame [D, 4, 3]."""
    return [("GLY", name, elem, "A", d + 1, tuple(quad[k])) for d, quad in enumerate(quads_xyz) for k, (name, elem) in enumerate((("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O")))]


# ---- 2: exact angles ----------------------------------------------------------------------------------------------------------------------------------------------------
EXACT_BINS = (4, 36, 72, 360)
EXACT_THETAS = (180, 0, 90, -90)


def exact_frames(mirrored: bool) -> np.ndarray:
    """[4, 4, 3]: one frame per angle of EXACT_THETAS (integer coordinates), or their mirror images."""
    q = np.array([tc.built_integer(t) for t in EXACT_THETAS])
    return tc.mirrored(q) if mirrored else q


def exact_pinned(mirrored: bool, B: int) -> dict:
    """The mirror image negates the angle: +-90 swap, 180 and 0 stay (180 is its own negative on the circle)."""
    s = -1.0 if mirrored else 1.0
    return {"angles": [180.0, 0.0, -90.0, 90.0] if mirrored else [180.0, 0.0, 90.0, -90.0], "states": [2, 1, 3, 1] if mirrored else [2, 1, 1, 3],
            "cossin": [[-1.0, 0.0], [1.0, 0.0], [0.0, s], [0.0, -s]], "bins": [0, B // 2, B // 4, 3 * B // 4] if mirrored else [0, B // 2, 3 * B // 4, B // 4]}


# ---- 3: the sign of the sine --------------------------------------------------------------------------------------------------------------------------------------------
TINY = (0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022, -(2.0 ** -1022), 1e-200, -1e-200)


def with_p3(u: float, v: float) -> np.ndarray:
    q = tc.built(0.0)
    q[3] = (u, v, 1.0)
    return q


def sine_frames() -> np.ndarray:
    """[16, 4, 3]: p3 = (u, v, 1) for u = 1, then u = -1, v over TINY: x = u, y = v, h = 1, so c = u and s = v -- subnormal, signed, or a zero."""
    return np.array([with_p3(u, v) for u in (1.0, -1.0) for v in TINY])


# ---- 4: the cosine threshold --------------------------------------------------------------------------------------------------------------------------------------------
def cosine_frames() -> np.ndarray:
    """[9, 4, 3]: p3 = (u, sqrt(0.75), 1), u = -0.5 and its four neighbours on either side: c = u / h passes through -0.5."""
    us = [-0.5]
    for _ in range(4):
        us = [math.nextafter(us[0], -math.inf)] + us + [math.nextafter(us[-1], math.inf)]
    return np.array([with_p3(u, math.sqrt(0.75)) for u in us])


# ---- 5: the grid ----------------------------------------------------------------------------------------------------------------------------------------------------------
GRID = np.arange(-179, 181)


def grid_frames(shift: float) -> np.ndarray:
    """One built torsion per frame: the angles -179 .. 180 (shift 0: each on an edge of the 1-degree bins), or -178.5 .. 179.5 (shift 0.5: none near an edge)."""
    return np.array([tc.built(float(t) + shift) for t in (GRID if shift == 0.0 else GRID[:-1])])


# ---- 6: the wave-matched maps -------------------------------------------------------------------------------------------------------------------------------------------
MATCH_FRAMES = (63, 64, 65, 129)


def matched_case(base: np.ndarray, quads: np.ndarray, F: int, line) -> dict:
    """F jittered frames of base (seed 100 + F, the rule of the F.. cases of tests/test_torsion_gpu.py; the margins and the seed rule are torsion_cases'), with the
    three atoms `line` (the first three of a torsion that is in a pair of the maps) on a line of integer points in frame 2 and in the last frame: every torsion
    through them is undefined there, so lanes drop out of the ballot -- in a full wave and in the partial last one."""
    name, seed = f"match_F{F}", 100 + F
    for s in range(seed, seed + 10):
        frames = ts.jitter(base, F, s)
        for f in (2, F - 1):
            frames[f, list(line)] = tc.COLLINEAR[:3] + 10.0
        if tc.clear(frames, quads, (36,)):
            if s != seed:
                tc.SKIPPED_SEEDS.append((name, seed))
            assert len(tc.SKIPPED_SEEDS) <= 1, tc.SKIPPED_SEEDS
            c = tc.case(name, frames, quads, (36,))
            c["collinear"] = (2, F - 1)
            return c
    raise AssertionError(f"{name}: no seed in {seed} .. {seed + 9} clears the margins")


KEY_ZERO_FRAMES = 66


def key_zero_case(F: int = KEY_ZERO_FRAMES) -> dict:
    """Two built torsions on eight atoms and the pair (0, 1) in one group: both at -175 degrees in most frames -- bin (0, 0) of 36, the key 0 that a lane outside
    the ballot carries too -- with torsion 1 at 65 degrees in the frames 2, 7, 12, .. (another key), and torsion 0 undefined (p0 = p1) in frame 3 and in the
    last frame.  The second wave holds frame 64 (key 0), the undefined frame 65 and 62 lanes past the frames: a wave that counted its inactive lanes would add
    them to bin (0, 0)."""
    q = np.zeros((F, 2, 4, 3))
    for f in range(F):
        q[f, 0] = tc.built(-175.0)
        q[f, 1] = tc.built(65.0 if f % 5 == 2 else -175.0)
        if f in (3, F - 1):
            q[f, 0, 0] = q[f, 0, 1]
    frames = np.ascontiguousarray(q.reshape(F, 8, 3))
    frames.setflags(write=False)
    return {"quads_xyz": q, "frames": frames, "quads": np.arange(8, dtype="<u4").reshape(2, 4), "pairs": np.array([[0, 1, 0]], "<u4"), "undefined": (3, F - 1)}
