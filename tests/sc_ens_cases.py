"""Case generators for shape complementarity across the frames of an ensemble (arp_sc_ensemble).  No product imports:
tests/test_sc_ens_host.py shows on the CPU, with the sequential restatement, that the cases with a purpose of their own reach it;
tests/test_sc_ens_gpu.py runs them on the device against the single-frame call, frame by frame.

An ensemble case is (xyz [F, n, 3], r [n], mol [n], settings) with the settings under the restatement's names (sc_edge_cases.DEFAULTS).
frame(case, f) is frame f as a single-frame input of sc_edge_cases' kind.

stats_reference() restates arp_sc_dot_stats in numpy, summation order included (include/arpeggia_amd.h): lane t of 256 adds the trimmed
dots at positions t, t + 256, ... of the segment in increasing position starting from +0.0, and the partial sums are folded
p[t] += p[t + h] for h = 128, 64, ..., 1."""
from __future__ import annotations

import numpy as np

import sc_edge_cases as E

TRIMMED, BURIED = 8, 4
STATUS = ("ok", "no_dots", "coincident", "sampling_limit")


def _stack(inp: dict) -> np.ndarray:
    return np.stack([inp["x"], inp["y"], inp["z"]], 1)


def frame(case, f: int) -> dict:
    xyz, r, mol, _ = case
    return {"x": xyz[f, :, 0].copy(), "y": xyz[f, :, 1].copy(), "z": xyz[f, :, 2].copy(), "r": r.copy(), "mol": mol.copy()}


def _rotation() -> np.ndarray:
    a, b = 0.7, -1.1  # about z, then about x
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    return rx @ rz


def six_frames(n_atoms: int = 600):
    """The halves as frame 0; molecule 1 lifted 0.3 A; Gaussian jitter of 0.2 A; the frame rotated about its centroid; the frame shifted
    300 A (a frame of its own origin: with one box around all frames the cells would coarsen); frame 0 again."""
    h = E.halves(n_atoms)
    x0 = _stack(h)
    lifted = x0.copy()
    lifted[h["mol"] == 1, 2] += 0.3
    jitter = x0 + np.random.default_rng(0x5CE5).normal(0.0, 0.2, x0.shape)
    c = x0.mean(0)
    rotated = (x0 - c) @ _rotation().T + c
    shifted = x0 + np.array([300.0, 0.0, 0.0])
    return np.stack([x0, lifted, jitter, rotated, shifted, x0.copy()]), h["r"], h["mol"], dict(E.DEFAULTS)


COINCIDENT_PAIR = (7, 31)  # two atoms of molecule 0 put on one point in the coincident frame (checked by the host test)


def failing_frames(n_atoms: int = 300):
    """Five frames for passes of three: good, NO_DOTS (the molecules 50 A apart), good (lifted), COINCIDENT (two atoms of molecule 0 on
    one point), good (jitter).  The failures sit between good frames, one in each pass."""
    h = E.halves(n_atoms)
    x0 = _stack(h)
    apart = x0.copy()
    apart[h["mol"] == 1, 2] += 50.0
    lifted = x0.copy()
    lifted[h["mol"] == 1, 2] += 0.3
    i, j = (int(k) for k in np.flatnonzero(h["mol"] == 0)[list(COINCIDENT_PAIR)])
    same = x0.copy()
    same[j] = same[i]
    jitter = x0 + np.random.default_rng(0xFA11).normal(0.0, 0.2, x0.shape)
    return (np.stack([x0, apart, lifted, same, jitter]), h["r"], h["mol"], dict(E.DEFAULTS)), (i, j)


def no_trim_frame():
    """One frame in which both surfaces have dots and surface 0 has no trimmed dot (surface 1 has one): two small clumps whose buried dots
    all lie within the band of an open dot.  Measured with the restatement: dots [2798, 890], trimmed [0, 1]."""
    c = E.cluster(22, [1.9, 1.8, 1.7, 1.9, 1.8, 1.7, 1.9, 1.8], [1.8, 1.7], 3.5, 0.8)
    return _stack(c)[None], c["r"], c["mol"], dict(E.DEFAULTS)


def shifted_pair(case):
    """A two-frame ensemble of a single-frame case: frame 1 is frame 0 shifted by 0.5 A on each axis."""
    inp, st = case
    x0 = _stack(inp)
    return np.stack([x0, x0 + 0.5]), inp["r"], inp["mol"], dict(st)


def wide_and_compact():
    """wide_box("three_level") -- 1.5 A cell lists of more than 1024^2 cells, a third scan level inside a slab -- next to a frame in which
    the far atom sits 40 A from the centre instead."""
    inp, st = E.wide_box("three_level")
    x0 = _stack(inp)
    near = x0.copy()
    near[-1] = np.round(x0[:-1].mean(0)) + 40.0
    return np.stack([x0, near]), inp["r"], inp["mol"], dict(st)


# ---- the statistics kernel on synthetic dots
def stats_reference(seg_start, flags, area, nn_dist, score, other) -> dict:
    """arp_sc_dot_stats in numpy: the sums in the stated order, the medians by np.partition (element k // 2)."""
    seg_start = np.asarray(seg_start, dtype=np.int64)
    n_seg = len(seg_start) - 1
    trimmed = (np.asarray(flags) & TRIMMED) != 0
    out = {k: np.zeros(n_seg) for k in ("trimmed_area", "d_mean", "d_median", "s_mean", "s_median")}
    out["n_all_dots"] = np.diff(seg_start).astype(np.uint64)
    out["n_trimmed_dots"] = np.array([trimmed[seg_start[s]:seg_start[s + 1]].sum() for s in range(n_seg)], dtype=np.uint64)

    def ordered_sum(v, m):
        p = np.zeros(256)
        for t in range(min(256, len(v))):
            acc = 0.0
            for x in v[t::256][m[t::256]]:
                acc = acc + x
            p[t] = acc
        h = 128
        while h >= 1:
            p[:h] = p[:h] + p[h:2 * h]
            h //= 2
        return p[0]

    for s in range(n_seg):
        sl = slice(seg_start[s], seg_start[s + 1])
        m = trimmed[sl]
        k = int(m.sum())
        out["trimmed_area"][s] = ordered_sum(np.asarray(area)[sl], m)
        o = int(other[s])
        if k == 0 or not trimmed[seg_start[o]:seg_start[o + 1]].any():
            continue
        d, sc = np.asarray(nn_dist)[sl], np.asarray(score)[sl]
        out["d_mean"][s] = ordered_sum(d, m) / k
        out["s_mean"][s] = -(ordered_sum(-sc, m) / k)
        out["d_median"][s] = np.partition(d[m], k // 2)[k // 2]
        out["s_median"][s] = np.partition(sc[m], k // 2)[k // 2]
    return out


def stats_cases() -> dict:
    """name -> (seg_start, flags, area, nn_dist, score, other).  Two-segment cases pair the segments with each other."""
    rng = np.random.default_rng(0x57A7)
    c = {}

    def dots(n, p_trim=0.6):
        fl = np.where(rng.random(n) < p_trim, TRIMMED | BURIED, rng.integers(0, 8, n)).astype(np.uint32)  # trimmed interleaved with the rest
        return fl, rng.random(n) * 0.07, rng.random(n) * 3.0, np.clip(rng.normal(0.0, 0.6, n), -0.999, 0.999)

    def pair(fl, a, d, s, n0):
        return np.array([0, n0, len(fl)]), fl, a, d, s, np.array([1, 0])

    def join(*parts):
        return tuple(np.concatenate(v) for v in zip(*parts))

    partner = dots(40)
    for k in (0, 1, 2, 3):  # segments of k trimmed dots among 5 untrimmed ones
        fl, a, d, s = dots(5 + k, 0.0)
        fl[:] = BURIED
        fl[rng.permutation(5 + k)[:k]] = TRIMMED | BURIED
        c[f"trimmed_{k}"] = pair(*join((fl, a, d, s), partner), 5 + k)
    for n in (255, 256, 257, 70001):  # around the block width; many strides of the lanes
        c[f"len_{n}"] = pair(*join(dots(n), partner), n)
    fl, a, d, s = dots(1000, 1.0)
    d[:] = 1.25
    s[:] = -0.5
    c["all_equal"] = pair(*join((fl, a, d, s), partner), 1000)
    fl, a, d, s = dots(999, 1.0)  # neighbours in the last mantissa bit: the select must read all 64 key bits
    d[:] = np.nextafter(1.0, 2.0)
    d[::2] = 1.0
    d[::3] = np.nextafter(np.nextafter(1.0, 2.0), 2.0)
    s[:] = np.where(np.arange(999) % 2, -0.25, np.nextafter(-0.25, 0.0))
    c["last_bit"] = pair(*join((fl, a, d, s), partner), 999)
    fl, a, d, s = dots(600, 0.8)  # both signs around zero, +0 and -0 themselves, and the clamp values
    s[:] = rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 0.999, -0.999, 0.5, -0.5]), 600)
    c["signs"] = pair(*join((fl, a, d, s), partner), 600)
    fl, a, d, s = dots(601, 1.0)  # the median itself is a zero, the zeros of one sign only (the sign is then defined)
    s[:] = np.concatenate([np.full(200, -0.3), np.full(201, -0.0), np.full(200, 0.4)])[rng.permutation(601)]
    c["median_zero"] = pair(*join((fl, a, d, s), partner), 601)
    n_tiny = 1000  # 1 000 tiny segments in one call, paired (2 k, 2 k + 1); some are empty, some have no trimmed dot
    lens = rng.integers(0, 7, n_tiny)
    c["tiny_1000"] = (np.concatenate([[0], np.cumsum(lens)]), *dots(int(lens.sum()), 0.5), np.arange(n_tiny) ^ 1)
    fl, a, d, s = dots(300)
    fl2, a2, d2, s2 = dots(50, 0.0)
    fl2[:] &= ~np.uint32(TRIMMED)  # the other segment has no trimmed dot: zeros, with the counts and the area kept
    c["other_empty"] = pair(*join((fl, a, d, s), (fl2, a2, d2, s2)), 300)
    return c
