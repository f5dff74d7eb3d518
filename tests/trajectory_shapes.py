"""Frames that drift, tumble, swell, collapse and go flat: seeded, deterministic generators for the ensemble paths (the frames
of a pass are the models of one grid, DevAtoms::per_model), and a plain restatement of the grid sizing so that a CPU test can show that every
case reaches the mechanism it is named for.  No GPU code and no product imports.

Every generator takes a base [N, 3] f64 array (or [F, N, 3]: a base per frame, for topologies whose frames follow a schedule of their own) and
returns [F, N, 3] f64.  What the per-model grid does with them (arpeggia_amd/csrc/grid.inl):
k_model_bounds reduces a box per frame as f32 values rounded outwards; setup_block takes the largest extent per axis over the frames, gives every
frame its own origin (its box's min corner) and its own midpoint for the f32 records (model_org); every frame owns a z slab of nz layers followed
by one empty separator layer; grid_setup coarsens the cells (edge x 2^(1/3) per step) while frames x nx x ny x (nz + 1) exceeds the workspace's
cell capacity.
"""
from __future__ import annotations

import numpy as np

SIGMA = 0.3  # A: the jitter every other ensemble test uses
DRIFT_REACH = 1.6e5  # A: the last frame's translation (norm); components 0.6, -0.64, 0.48 of it: all three between 2^16 and 2^17
DRIFT_DIRECTION = np.array([0.6, -0.64, 0.48])  # (norm 1; mixed signs)
SWELL_FACTOR = 24.0
COARSEN = 1.2599210498948732  # grid.inl grid_setup: the edge's factor per coarsening step


def centroid(xyz: np.ndarray) -> np.ndarray:
    return np.asarray(xyz, np.float64).mean(0)


def per_frame(base: np.ndarray, F: int) -> np.ndarray:
    """[F, N, 3]: the base of every frame (a copy)."""
    base = np.asarray(base, np.float64)
    if base.ndim == 2:
        return np.repeat(base[None], F, 0)
    assert base.ndim == 3 and len(base) >= F
    return base[:F].copy()


def jitter(base: np.ndarray, F: int, seed: int, sigma: float = SIGMA) -> np.ndarray:
    """base + a seeded normal step per atom and frame: the frames of the existing tests (all boxes equal to within about 1 A)."""
    b = per_frame(base, F)
    return b + np.random.default_rng(seed).normal(scale=sigma, size=b.shape)


def drift(base: np.ndarray, F: int, seed: int = 1) -> np.ndarray:
    """Frame f = base translated by DRIFT_REACH (f / (F - 1))^3 along DRIFT_DIRECTION; frame 0 stays where it is.
    Aims at: the per-frame origin and midpoint (model_org), the f32 box codes rounded outwards, and records taken against the frame's OWN
    midpoint -- at 10^5 A an f32 has a spacing of 2^-7 A, so a record against a shared midpoint is off by about 8e-3 A, which moves d^2 by far
    more than the f32 band of k_sasa or the prefilter margin of the pair kernels."""
    assert F >= 2
    t = DRIFT_REACH * (np.arange(F, dtype=np.float64) / (F - 1)) ** 3
    return per_frame(base, F) + t[:, None, None] * DRIFT_DIRECTION[None, None, :]


def principal_axis(base: np.ndarray) -> np.ndarray:
    c = np.asarray(base, np.float64) - centroid(base)
    return np.linalg.svd(c, full_matrices=False)[2][0]


def rotation_to(u: np.ndarray, v: np.ndarray) -> np.ndarray:
    """A rotation matrix that turns unit vector u into unit vector v (Rodrigues; u != -v)."""
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    w, c = np.cross(u, v), float(np.dot(u, v))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + K + K @ K / (1.0 + c)


def random_rotation(rng) -> np.ndarray:
    q = rng.normal(size=4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def tumble(base: np.ndarray, F: int, seed: int = 2) -> np.ndarray:
    """A rigid rotation per frame about the centroid.  Frames 0, 1, 2 lay the topology's principal axis along x, y and z (then a seeded turn
    about that axis); the others are seeded uniform rotations.  On an elongated topology the longest axis changes from frame to frame.
    Aims at: the grid sized per axis over ALL frames (setup_block: ext[k] = the maximum over the frames, a different frame for different k)."""
    assert F >= 3
    rng = np.random.default_rng(seed)
    bases = per_frame(base, F)
    c0, u = centroid(bases[0]), principal_axis(bases[0])
    out = np.empty(bases.shape)
    for f in range(F):
        base = bases[f]
        if f < 3:
            e = np.eye(3)[f]
            phi = rng.uniform(0.0, 2.0 * np.pi)
            K = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
            spin = np.eye(3) + np.sin(phi) * K + (1.0 - np.cos(phi)) * (K @ K)
            R = spin @ rotation_to(u if np.dot(u, e) > -0.9 else -u, e)
        else:
            R = random_rotation(rng)
        out[f] = (base - c0) @ R.T + c0
    return out


def scaled(frame: np.ndarray, factor: float) -> np.ndarray:
    c = centroid(frame)
    return (np.asarray(frame, np.float64) - c) * factor + c


def swell(base: np.ndarray, F: int, at: int, factor: float = SWELL_FACTOR, seed: int = 3) -> np.ndarray:
    """Jittered frames; frame `at` scaled about its centroid by `factor`.
    Aims at: the coarsening loop of grid_setup -- at the uncoarsened edge nx ny (nz + 1) F exceeds the workspace's cell capacity, the cells
    grow, and every other frame of the pass lives in a few coarse cells (long slot windows in k_sasa and k_neighbor_sum)."""
    out = jitter(base, F, seed)
    out[at] = scaled(out[at], factor)
    return out


STRETCH_REACH = 3.0e4  # A: how far the second half of the stretched frame moves (along DRIFT_DIRECTION)


def stretch(base: np.ndarray, F: int, at: int, seed: int = 7) -> np.ndarray:
    """Jittered frames; in frame `at` the second half of the atoms (by index) moves STRETCH_REACH away, each half staying as it is.
    Aims at: the bound of k_sasa's f32 band, C >= |record coordinate|.  Unlike the swollen frame, this one keeps its
    neighbours, so its atoms are tested at record coordinates of 10^4 A: a grid sized from another frame's extent would take the band from a
    C of a few tens of angstroms while the records carry f32 steps of 10^-3 A."""
    out = jitter(base, F, seed)
    n = out.shape[1]
    out[at, n // 2:] += STRETCH_REACH * DRIFT_DIRECTION
    return out


def collapse_factor(base: np.ndarray, reach: float) -> float:
    """The scale at which the largest distance between two atoms of `base` is 0.9 x reach."""
    b = per_frame(base, 1)[0]
    # (the diameter is at most twice the largest distance from the centroid: good enough for a factor)
    return 0.9 * reach / (2.0 * float(np.linalg.norm(b - centroid(b), axis=1).max() + 3.0 * SIGMA))


def collapse(base: np.ndarray, F: int, at: int, reach: float, point: bool = False, seed: int = 4) -> np.ndarray:
    """Jittered frames; frame `at` scaled about its centroid until every atom is within `reach` (the smallest R_i + R_j of the call) of every
    other -- or, with point=True, all of its atoms on one point.
    Aims at: the list flush of k_sasa (more than 256 list entries per home, every one a burier candidate), one cell holding a whole frame,
    and at one point d^2 = |s_k|^2 R_i^2 against R_j^2: the f32 band around equality on every test."""
    out = jitter(base, F, seed)
    out[at] = centroid(out[at])[None] if point else scaled(out[at], collapse_factor(base, reach))
    return out


def flat(base: np.ndarray, F: int, axes: str, seed: int = 5, thickness: float = 0.5) -> np.ndarray:
    """Jittered frames squeezed along `axes` ("z", "yz" or "xyz"): even frames to extent zero, odd frames to at most `thickness` A (below
    one cell).  Aims at: nz == 1 (then ny == 1, then nx == 1) -- every slab is one layer plus its separator, so the frames above and below
    a home's layer are one layer away: what the separator is for."""
    out = jitter(base, F, seed)
    for f in range(F):
        for ax in axes:
            k = "xyz".index(ax)
            col = out[f, :, k]
            lo, hi = float(col.min()), float(col.max())
            out[f, :, k] = (lo + hi) / 2.0 if f % 2 == 0 else (lo + hi) / 2.0 + (col - (lo + hi) / 2.0) * (thickness / max(hi - lo, 1e-9)) * 0.999
    return out


def mixed(base: np.ndarray, F: int, reach: float, seed: int = 6) -> np.ndarray:
    """All of the above and plain jitter in one ensemble of F >= 16 frames, in a seeded shuffled order: three drifted frames (to the full
    reach), three tumbled, one swollen, one collapsed, one on a point, flat in z (two), in y and z, in all three, the rest jittered."""
    assert F >= 16
    base = per_frame(base, 1)[0] if np.asarray(base).ndim == 3 else np.asarray(base, np.float64)
    parts = [drift(base, 4, seed)[1:], tumble(base, 3, seed + 1), swell(base, 1, 0, seed=seed + 2), collapse(base, 1, 0, reach, seed=seed + 3),
             collapse(base, 1, 0, reach, point=True, seed=seed + 4), flat(base, 2, "z", seed + 5), flat(base, 1, "yz", seed + 6),
             flat(base, 1, "xyz", seed + 7)]
    n = sum(len(p) for p in parts)
    parts.append(jitter(base, F - n, seed + 8))
    frames = np.concatenate(parts)
    order = np.random.default_rng(seed).permutation(F)
    return frames[order]


def positions(F: int) -> tuple:
    """Where the one special frame of swell / collapse goes: first, in the middle, last."""
    return (0, F // 2, F - 1)


# ---- the grid sizing restated ----------------------------------------------------------------------------------------------------------------
def f32_down(v):
    v = np.asarray(v, np.float64)
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float64)


def f32_up(v):
    v = np.asarray(v, np.float64)
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float64)


def frame_extents(frames: np.ndarray, f32_coordinates: bool = False) -> np.ndarray:
    """[F, 3]: the extent of every frame's box as k_model_bounds / setup_block form it -- min rounded down and max rounded up to f32, the
    difference in f64.  f32_coordinates: the grid is built over the f64 images of the f32-rounded coordinates (the SASA grid; ens.inl k_ens_tile)."""
    frames = np.asarray(frames, np.float64)
    if f32_coordinates:
        frames = frames.astype(np.float32).astype(np.float64)
    return f32_up(frames.max(1)) - f32_down(frames.min(1))


def cell_capacity(n_atoms: int) -> int:
    """engine.cpp ensure_workspace for a workspace that is sized by this call: 8 cells per atom of capacity (n + n / 8, at least 1024) + 65 536.
    (A context keeps the largest workspace it ever needed: the GPU tests give the cases that must coarsen a context of their own.)"""
    cap = max(n_atoms + n_atoms // 8, 1024)
    return min(8 * cap + 65536, 0xFFFFFFF0)


def grid_sizing(ext, n_frames: int, n_atoms: int, cutoff: float, ncells_cap: int | None = None) -> dict:
    """grid.inl grid_setup for a packed input: ext = the per-axis extent (the maximum over the frames), n_atoms = the packed atoms of the pass.
    Returns edge, kx, nx, ny, nz, nzt and `steps`, the number of coarsening steps."""
    cap = cell_capacity(n_atoms) if ncells_cap is None else int(ncells_cap)
    ext = [float(e) if np.isfinite(e) and e >= 0.0 else 0.0 for e in ext]
    nm = max(int(n_frames), 1)
    if 2 * nm > cap:
        nm = cap // 2
    edge = abs(float(cutoff)) * (1.0 + 1e-6)
    if not edge > 1e-3:
        edge = 1e-3
    soft_cap = min(float(cap), max(0.35 * float(n_atoms), 4096.0))
    steps = 0
    while True:
        ny, nz = np.floor(ext[1] / edge) + 1.0, np.floor(ext[2] / edge) + 1.0
        kx = 4
        while kx > 1:
            nx = np.floor(ext[0] * kx / edge) + 1.0
            if nx * ny * (nz + 1.0) * nm <= soft_cap:
                break
            kx >>= 1
        nx = np.floor(ext[0] * kx / edge) + 1.0
        if nx * ny * (nz + 1.0) * nm <= float(cap):
            break
        assert steps < 512
        edge *= COARSEN
        steps += 1
    return {"edge": edge, "kx": kx, "nx": int(nx), "ny": int(ny), "nz": int(nz), "nzt": nm * (int(nz) + 1), "steps": steps, "cap": cap}


def sizing_of(frames: np.ndarray, n_selected: int, cutoff: float, f32_coordinates: bool = False, per: int | None = None, ncells_cap: int | None = None) -> dict:
    """grid_sizing for the pass that holds the first `per` frames (default: all) of `frames` ([F, m, 3]: the atoms that are in the grid)."""
    F = len(frames) if per is None else min(per, len(frames))
    ext = frame_extents(frames[:F], f32_coordinates).max(0)
    return grid_sizing(ext, F, F * n_selected, cutoff, ncells_cap)


def axis_owners(frames: np.ndarray, f32_coordinates: bool = False) -> list:
    """Per axis the frame whose extent is the largest."""
    return np.argmax(frame_extents(frames, f32_coordinates), axis=0).tolist()


def f32_spacing(v) -> np.ndarray:
    """The distance between neighbouring f32 values at |v|."""
    a = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def pair_counts_within(xyz: np.ndarray, R) -> np.ndarray:
    """Per atom the number of others with |c_i - c_j| < R_i + R_j, by brute force in f64 on the f32 coordinates (what fills k_sasa's list)."""
    c = np.asarray(xyz, np.float64).astype(np.float32).astype(np.float64)
    R = np.asarray(R, np.float32).astype(np.float64)
    d = np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1))
    near = d < (R[:, None] + R[None, :])
    np.fill_diagonal(near, False)
    return near.sum(1)


# ---- the cases both new test files use ---------------------------------------------------------------------------------------------------------
REACH = 5.6  # A: below the smallest R_i + R_j of any call here (two ProtOr carbonyl oxygens with the 1.4 A probe: 2 x 2.82)
SHAPES = ("drift", "tumble", "swell@first", "swell@mid", "swell@last", "stretch@mid", "collapse@first", "collapse@mid", "collapse@last", "point@mid",
          "flat_z", "flat_yz", "flat_xyz", "mixed")
MIXED_SLOTS = {"far": 2, "swollen": 6, "collapsed": 7, "point": 8, "flat_z": 9, "flat_yz": 11, "flat_xyz": 12}  # positions in mixed() before the shuffle


def make(name: str, base: np.ndarray, F: int = 16):
    """(frames [F, N, 3], {label: index of an extreme frame}) of a named case."""
    where = {"first": 0, "mid": F // 2, "last": F - 1}
    kind, _, pos = name.partition("@")
    if kind == "drift":
        return drift(base, F), {"far": F - 1, "home": 0}
    if kind == "tumble":
        return tumble(base, F), {"x": 0, "z": 2}
    if kind == "swell":
        return swell(base, F, where[pos]), {"swollen": where[pos]}
    if kind == "stretch":
        return stretch(base, F, where[pos]), {"stretched": where[pos]}
    if kind == "collapse":
        return collapse(base, F, where[pos], REACH), {"collapsed": where[pos]}
    if kind == "point":
        return collapse(base, F, where[pos], REACH, point=True), {"point": where[pos]}
    if kind.startswith("flat_"):
        return flat(base, F, kind[5:]), {"flat_even": 0, "flat_odd": 1}
    if kind == "mixed":
        order = np.random.default_rng(6).permutation(F)
        return mixed(base, F, REACH, seed=6), {k: int(np.flatnonzero(order == v)[0]) for k, v in MIXED_SLOTS.items()}
    raise KeyError(name)


def special_frame(name: str, F: int = 16):
    """The frame of a swell / stretch / collapse / point case that a forced split can leave alone in a pass (None for the other shapes)."""
    kind, _, pos = name.partition("@")
    return {"first": 0, "mid": F // 2, "last": F - 1}[pos] if pos else None


def forced_passes(name: str, F: int = 16) -> list:
    """Frames per pass of the forced runs: three passes with a partial last one, one frame per pass (every frame alone), and for a special
    frame at the end a split whose last pass holds that frame alone."""
    per3 = -(-F // 3)
    assert F % per3 != 0 and -(-F // per3) == 3
    out = [per3, 1]
    if special_frame(name, F) == F - 1:
        per = next(p for p in range(F - 1, 1, -1) if F % p == 1)
        out.append(per)
    return out


# ---- the two built topologies: the frame cap and the flat slabs ----------------------------------------------------------------------------------
CAP_FRAMES = 65535 + 6  # one full pass of the model ordinal range and a second pass of six frames
CAP_PERIOD = 7
AUTO_PASS_ATOMS = 1 << 21  # sasa_dev.cpp kEnsAutoAtoms, freq.inl kFreqAutoAtoms


def records(atoms: list) -> dict:
    """Topology records from [(resn, atom name, element, chain, resi, (x, y, z))] (tests/synth.py's columns; Structure.from_records takes them)."""
    import synth

    cols = {k: [] for k in ("x", "y", "z", "occupancy", "serial", "resi", "name", "resn", "chain", "altloc", "icode", "element", "model_serial")}
    for k, (resn, name, elem, chain, resi, xyz) in enumerate(atoms):
        for c, v in (("x", xyz[0]), ("y", xyz[1]), ("z", xyz[2]), ("occupancy", 1.0), ("serial", k + 1), ("resi", resi), ("name", name), ("resn", resn),
                     ("chain", chain), ("altloc", ""), ("icode", ""), ("element", elem), ("model_serial", 0)):
            cols[c].append(v)
    return synth._finish(cols)


def cap_topology() -> dict:
    """15 atoms: GLY 1 and ALA 2 of chain A, SER 1 of chain B, on a loose 1.5 A zigzag; B lies 3.4 A above A, so its OG and A's carbonyl oxygens
    are a contact pair in every conformation."""
    names = [("GLY", 1, "A", [("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O")]), ("ALA", 2, "A", [("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C")]),
             ("SER", 1, "B", [("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C"), ("OG", "O")])]
    atoms, k = [], 0
    for resn, resi, chain, members in names:
        for name, elem in members:
            if chain == "A":
                xyz = (1.45 * k, 0.7 * (k % 2), 0.3 * (k % 3))
            else:
                j = k - 9
                xyz = (2.0 + 1.45 * j, 0.6 * (j % 2), 3.4 + 0.25 * (j % 3))
            atoms.append((resn, name, elem, chain, resi, xyz))
            k += 1
    return records(atoms)


def cap_conformations(rec: dict) -> np.ndarray:
    """[CAP_PERIOD, n, 3]: the topology with a seeded 0.3 A jitter per conformation and no translation: neighbouring frames differ, and their
    boxes overlap in box-relative coordinates -- a frame that saw the slab next to it would gain false burials and false contacts."""
    base = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    return jitter(base, CAP_PERIOD, seed=65535)


def cap_frames(conf: np.ndarray, F: int = CAP_FRAMES) -> np.ndarray:
    return conf[np.arange(F) % len(conf)]


FLAT_FRAMES = 200


def flat_topology() -> dict:
    """Four atoms in two chains (GLY A 1: N, CA; GLY B 1: C, O), at the buried arrangement."""
    buried = flat_arrangements()[0]
    spec = [("GLY", "N", "N", "A", 1), ("GLY", "CA", "C", "A", 1), ("GLY", "C", "C", "B", 1), ("GLY", "O", "O", "B", 1)]
    return records([(a, b, c, d, e, tuple(buried[k])) for k, (a, b, c, d, e) in enumerate(spec)])


def flat_arrangements() -> np.ndarray:
    """[2, 4, 3]: buried -- the four atoms within 1.2 A of each other; open -- the corners of a 5.5 A square in the yz plane.  Both are at most
    1.2 A wide in x and 5.5 A in y and z: below a quarter cell in x (kx = 4) and below one cell in y and z, so nx == ny == nz == 1."""
    buried = np.array([[0.0, 0.0, 0.0], [1.2, 0.5, 0.0], [0.3, 1.1, 0.6], [0.9, 0.2, 1.0]])
    open_ = np.array([[0.0, 0.0, 0.0], [1.2, 5.5, 0.0], [0.3, 0.0, 5.5], [0.9, 5.5, 5.5]])
    return np.stack([buried, open_])


def flat_frames(F: int = FLAT_FRAMES) -> np.ndarray:
    return flat_arrangements()[np.arange(F) % 2]
