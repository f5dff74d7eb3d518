"""Helpers of the buried-surface tests (arp_atom_sasa_groups, arp_structure_buried_sasa, arp_dsasa_ensemble): the split contract restated as
three runs of the atom-SASA restatement (tests/sasa_restatement.py: the union, group 1 alone, group 2 alone), the case inputs that
tests/test_bsa_host.py checks on the CPU and tests/test_bsa_gpu.py runs on the device, and the host-side statistics written out with Python
integers.  No product imports: the yardstick of the new kernel is never the new kernel."""
from __future__ import annotations

import math

import numpy as np

import sasa_edge_cases as edge
import sasa_restatement as sr

FOUR_PI = 4.0 * 3.141592653589793
PAIR_POINTS = (1, 63, 64, 65, 128, 257, 4095, 4096)  # one pass, the pass edge, more than four passes, 64 passes (bit 63 of every buried word)
PAIR_MASKS = ((1, 2), (2, 1), (3, 3), (1, 1))
COINCIDENT_N = (300, 600, 1100)
FILE_GROUPS = ("C/H,L", "H/L", "A,B/G", "/", "A,B/A,G", "C/")


def split_counts(x, y, z, R, group, sphere, homes=None):
    """The contract of the split kernel as three runs of sr.atom_counts.  group: u8 masks (0: out of the calculation).  homes: indices into
    the input arrays (default: every atom with a non-zero mask; each must have one).  Returns (count [3, len(homes)] int32: complex, group 1,
    group 2, with 0 where the home is not in the group; buried [len(homes)] int32)."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    R, group = np.asarray(R, np.float32), np.asarray(group, np.uint8)
    homes = np.flatnonzero(group) if homes is None else np.asarray(homes, np.int64)
    assert (group[homes] != 0).all()
    out = np.zeros((3, len(homes)), np.int32)
    for plane, members in enumerate((group != 0, (group & 1) != 0, (group & 2) != 0)):
        idx = np.flatnonzero(members)
        pos = np.full(len(group), -1, np.int64)
        pos[idx] = np.arange(len(idx))
        mine = members[homes]
        if mine.any():
            out[plane, mine] = sr.atom_counts(x[idx], y[idx], z[idx], R[idx], sphere, homes=pos[homes[mine]])
    return out, (out[1] + out[2] - out[0]).astype(np.int32)


def areas(R, counts, n_points) -> np.ndarray:
    """f32 areas of [3, m] counts (sr.sasa_from_counts per plane; count 0 gives +0.0)."""
    return np.stack([sr.sasa_from_counts(R, c, n_points) for c in counts])


def pair_on_z(n_points: int):
    """Two atoms on the z axis (point 0 of the lower one is the contact point), R = 2.0 and 2.5, centres 3.0 apart: each buries a cap of the
    other.  Returns x, y, z (f64), R (f32; use with probe 0)."""
    return np.array([1.5, 1.5]), np.array([-0.75, -0.75]), np.array([4.0, 7.0]), np.array([2.0, 2.5], np.float32)


def coincident_masks(n: int) -> dict:
    """The mask sets of the flush cases on edge.coincident(n): alternating, one group-1 atom among group-2 atoms, the reverse, and random masks
    from {0, 1, 2, 3} over three seeds."""
    out = {"alternating": (1 + (np.arange(n) % 2)).astype(np.uint8)}
    lone = np.full(n, 2, np.uint8)
    lone[n // 3] = 1
    out["lone1"] = lone
    out["lone2"] = (3 - lone).astype(np.uint8)
    for seed in (1, 2, 3):
        out[f"random{seed}"] = np.random.default_rng(1000 * n + seed).integers(0, 4, n).astype(np.uint8)
    return out


def coincident_homes(mask: np.ndarray) -> np.ndarray:
    """A few homes of every mask value present (first, middle, last of each)."""
    homes = []
    for g in (1, 2, 3):
        at = np.flatnonzero(mask == g)
        if len(at):
            homes += [at[0], at[len(at) // 2], at[-1]]
    return np.unique(np.array(homes, np.int64))


def random_masks(n: int, seed: int, with_zero: bool = True) -> np.ndarray:
    return np.random.default_rng(seed).integers(0 if with_zero else 1, 4, n).astype(np.uint8)


def halves_by_residue(resi) -> np.ndarray:
    """The artificial split of a one-chain structure: residue numbers up to the median are group 1, the rest group 2."""
    resi = np.asarray(resi)
    return np.where(resi <= np.median(resi), 1, 2).astype(np.uint8)


def f64_total(values) -> np.float32:
    """The f64 sum of f32 values in order (cumsum adds one by one), rounded to f32 once."""
    v = np.asarray(values, np.float32).astype(np.float64)
    return np.float32(np.cumsum(v)[-1] if len(v) else 0.0)


def dsasa_f32(total_c, total_1, total_2) -> np.float32:
    return np.float32(np.float32(np.float32(total_1) + np.float32(total_2)) - np.float32(total_c))


def buried_stats(n_frames: int, R, n_points: int, buried) -> dict:
    """The per-atom columns of the ensemble table from [F, m] integer buried points, with Python integers: a point is worth (4 pi R) R / n;
    mean = b S1 / n / F, std = b sqrt(F S2 - S1^2) / n / F, min / max = b c / n, every value one f64 chain rounded to f32 once (the formulas of
    arp_sasa_ensemble_stats); occupancy = frames with buried > 0 / F in f64."""
    buried = np.asarray(buried)
    F, m = buried.shape
    assert F == n_frames
    out = {k: np.zeros(m, np.float32) for k in ("buried_mean", "buried_std", "buried_min", "buried_max")}
    out["occupancy"] = np.zeros(m, np.float64)
    n, Ff = float(n_points), float(n_frames)
    for k in range(m):
        col = [int(c) for c in buried[:, k]]
        s1, s2 = sum(col), sum(c * c for c in col)
        d = n_frames * s2 - s1 * s1
        assert d >= 0
        r = float(np.float32(R[k]))
        b = (FOUR_PI * r) * r
        out["buried_mean"][k] = np.float32(b * float(s1) / n / Ff)
        out["buried_std"][k] = np.float32(b * math.sqrt(float(d)) / n / Ff)
        out["buried_min"][k] = np.float32(b * float(min(col)) / n)
        out["buried_max"][k] = np.float32(b * float(max(col)) / n)
        out["occupancy"][k] = sum(c > 0 for c in col) / Ff
    return out


def crowded_homes(x, y, z, R, group, above: int = 256, per_group: int = 24):
    """Neighbour counts among the atoms with a non-zero mask (what fills the kernel's list), and per group the member homes with more than
    `above` neighbours that have the fewest of them (the likeliest to keep open points).  Returns (nb [n], {1: homes, 2: homes})."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    R, group = np.asarray(R, np.float32), np.asarray(group, np.uint8)
    grid = np.flatnonzero(group)
    nb = np.zeros(len(group), np.int64)
    nb[grid] = edge.neighbour_counts(x[grid], y[grid], z[grid], R[grid])
    homes = {}
    for g in (1, 2):
        crowded = np.flatnonzero((nb > above) & ((group & g) != 0))
        homes[g] = np.sort(crowded[np.argsort(nb[crowded], kind="stable")[:per_group]])
    return nb, homes
