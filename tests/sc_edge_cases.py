"""Case generators for shape complementarity off its default settings and past one wave of latitudes.  No product imports:
tests/test_sc_edge_host.py runs these cases through the sequential restatement (tests/sc_restatement.c) on the CPU and asserts, from the
restatement's reach counters, that each case gets where it is named for; tests/test_sc_edge_gpu.py runs them on the device.

A case is (inp, settings): inp = {"x", "y", "z", "r", "mol"[, "serial"]} as plain arrays, settings = the restatement's keyword names
(rp, density, band, sep, w); api_settings() renames them for arp_sc_settings.  Every case is sized so that the restatement, which is
quadratic in the dots of the interface, takes about 2 s at the most (the measured times are in tests/test_sc_edge_host.py).

cell_dims() restates the geometry of the device's cell lists (sc.cpp / sc.inl sc_cells: pad = r_max + 2 rp + 1 on every side,
edge = max(edge_req, longest axis / 128), n = (int)(ext / edge) + 1 per axis) so that the wide_box cases can be placed at the two sizes
that matter: more than 1024^2 cells (a third level of the device scan) and the 128-cells-per-axis cap."""
from __future__ import annotations

import numpy as np

import sc_restatement as R
import synth

DEFAULTS = dict(R.SETTINGS)
SPHERE_AREA_RTOL = 5e-4  # two_big_spheres: summed dot area against 4 pi r^2 (the restatement itself is off by +1.32e-4; a lost latitude costs 1.4e-2)
TIE_ORDERS = (None, 1, 2)  # d2_ties: the generator's own order of the atoms and two permutations of it
API_KEYS = dict(rp="probe_radius", density="dot_density", band="peripheral_band", sep="separation_cutoff", w="gaussian_w")


def api_settings(st: dict) -> dict:
    return {API_KEYS[k]: v for k, v in st.items()}


def _inp(xyz, r, mol, serial=None) -> dict:
    xyz = np.asarray(xyz, dtype=np.float64)
    d = {"x": xyz[:, 0].copy(), "y": xyz[:, 1].copy(), "z": xyz[:, 2].copy(), "r": np.asarray(r, dtype=np.float64).copy(),
         "mol": np.asarray(mol, dtype=np.uint8).copy()}
    if serial is not None:
        d["serial"] = np.asarray(serial, dtype=np.int64).copy()
    return d


_HALVES = {}


def halves(n_atoms: int, gap: float = 0.6) -> dict:
    """The S2 ball of tests/synth.py cut at its middle plane (the lower half is molecule 0, the upper half, moved up by `gap`, molecule
    1) with the Lawrence & Colman radii of tests/golden/sc_radii.csv, 1.8 where the table has none.  A fresh copy on every call."""
    if (n_atoms, gap) not in _HALVES:
        rec = synth.gen_s2(n_atoms)
        z = rec["z"].copy()
        mol = (z > np.median(z)).astype(np.uint8)
        z[mol == 1] += gap
        table, cache = R.radius_table(), {}
        r = np.array([cache.setdefault(k, R.sc_radius(k[0].decode(), k[1].decode(), 0.0, table) or 1.8) for k in zip(rec["resn"], rec["name"])])
        _HALVES[(n_atoms, gap)] = {"x": rec["x"].copy(), "y": rec["y"].copy(), "z": z, "r": r, "mol": mol}
    return {k: v.copy() for k, v in _HALVES[(n_atoms, gap)].items()}


def cluster(seed: int, radii0, radii1, half: float, gap: float, overlap: float = 0.75) -> dict:
    """Two clumps of overlapping spheres, molecule 0 below z = 0 and molecule 1 above z = gap: each atom is drawn in a box of half-width
    `half` and kept when it lies at least overlap (r_i + r_j) from every atom before it (so no sphere contains another: overlap
    (r_i + r_j) > |r_i - r_j| for the radii used here).  Coordinates have three decimals."""
    rng = np.random.default_rng(seed)
    xyz, rad, mol = [], [], []
    for m, radii in enumerate((radii0, radii1)):
        for r in radii:
            for _ in range(100000):
                p = rng.uniform(-half, half, 3)
                p[2] = -abs(p[2]) if m == 0 else gap + abs(p[2])
                p = np.round(p, 3)
                if all(np.linalg.norm(p - q) >= overlap * (r + s) for q, s in zip(xyz, rad)):
                    break
            else:
                raise RuntimeError("cluster: no room")
            xyz.append(p); rad.append(r); mol.append(m)
    return _inp(np.array(xyz), rad, mol)


# ---- latitudes past one wave.  The latitude arc of a contact atom has about angle * r * sqrt(density) samples with angle <= pi, that
# of a probe about angle * rp * sqrt(density) with a shorter arc.
def lat_chunks_contact() -> dict:
    c = {}
    # density raised: r = 0.9 stays below 64 latitudes (at most 31), r = 2.0 / 2.5 passes 64 (at most 69 / 86), r = 5.0 passes 128
    c["density"] = (cluster(11, [5.0, 2.0, 0.9, 2.5, 2.0, 0.9, 2.0], [2.0, 0.9, 2.5, 2.0, 1.8, 0.9], 4.5, 1.0), dict(DEFAULTS, density=120.0, sep=12.0))
    # density kept: radii about 6 A pass 64 (at most 73), the 11.5 A atom passes 128 (at most 140), the small ones stay far below
    c["radii"] = (cluster(12, [11.5, 6.0, 1.8, 5.5, 1.9, 6.2], [6.0, 1.8, 5.8, 1.7, 6.1], 12.0, 1.5), dict(DEFAULTS, sep=30.0))
    return c


def concave_inputs() -> dict:
    """Two triangles of r = 1.7 atoms, one per molecule, wide enough (side about 8.9 A) that a probe of 3.5 A sits low between its three
    atoms (height about 0.9 A): the latitude arc of a probe runs from the direction of one of its atoms to its south pole, the lower the
    probe the nearer to pi / 2.  A low probe has a mirror image on the other side of its atoms' plane, 1.8 A away, which is a near of it
    and cuts every dot around its south pole -- the last latitudes, those of the second chunk.  Atom 7, 5.4 A over the second triangle,
    collides with the upper probe of that triangle only, so the lower one keeps its south pole.  Atom 3 under the first triangle removes
    both of its low probes and gives further triplets with higher probes and shorter arcs."""
    xyz = [[5.1, 0.1, 0.05], [-2.6, 4.4, -0.1], [-2.5, -4.45, 0.08], [0.4, 0.3, -3.0],
           [-5.05, 0.15, 5.5], [2.55, -4.4, 5.6], [2.6, 4.45, 5.45], [0.2, -0.1, 10.9]]
    return _inp(xyz, [1.7, 1.7, 1.7, 1.9, 1.7, 1.7, 1.7, 1.7], [0, 0, 0, 0, 1, 1, 1, 1])


CONCAVE_POINTS = ((3.5, 180.0), (3.5, 190.0), (3.5, 200.0))  # (rp, density)


def lat_chunks_concave() -> dict:
    # the arc is at most pi / 2 long, so rp sqrt(density) must pass 64 / (pi / 2) = 40.7: at rp = 3.5 a density above 136
    return {f"rp{rp}_d{int(d)}": (concave_inputs(), dict(DEFAULTS, rp=rp, density=d, sep=14.0)) for rp, d in CONCAVE_POINTS}


def two_big_spheres() -> tuple:
    """Two atoms of radius 6, one per molecule, 13.5 A apart on z: neither has a same-molecule neighbour, so each whole sphere is
    sampled, over 73 latitudes (two chunks of 64).  The one analytic anchor of the chunked path: the areas sum to 4 pi r^2 per atom."""
    return _inp([[0.0, 0.0, 0.0], [0.0, 0.0, 13.5]], [6.0, 6.0], [0, 1]), dict(DEFAULTS, sep=20.0)


# ---- sep as a binding bound (sep < r_i + r_j + 2 rp)
def sep_binding() -> dict:
    c = {"sep5.0": (halves(600), dict(DEFAULTS, sep=5.0)), "sep6.5": (halves(600), dict(DEFAULTS, sep=6.5))}
    # radii of 2.5 A at the default sep: 2 (r_max + rp) + margin = 8.41 > 8, the second branch of the atoms' cell edge
    h = halves(60)
    h["r"][:] = 2.5
    c["r2.5"] = (h, dict(DEFAULTS))
    return c


def burial_beyond_sep() -> tuple:
    """A burying atom farther away than sep.  Atom 0 (molecule 0, r = 2.5) is attended through atom 1 of molecule 1, 3.5 A away, at
    sep = 4; atom 2 of molecule 1 (r = 2.5) lies 7.5 A away along x, inside r_0 + r_2 + 2 rp = 8.4, and buries the cap of atom 0's
    dots that faces it.  On the device that atom is found only because the atoms' cell edge is max(sep, 2 (r_max + rp) + margin) = 8.41:
    with cells of edge sep it would lie two cells away.  (At a dense interface a nearer atom buries the same dots, so the halves at
    sep = 5 cannot tell.)  Atom 2 itself is Far and emits nothing."""
    return _inp([[0.0, 0.0, 0.0], [0.3, 3.5, 0.2], [7.5, 0.4, 0.3]], [2.5, 1.0, 2.5], [0, 1, 1]), dict(DEFAULTS, sep=4.0)


def sep_edge() -> dict:
    """On-axis placements with dyadic coordinates: every d^2 is exact in f64.
    other_*: one atom per molecule (r = 2.5) at d = sep and one step inside.  Buried is d^2 < sep^2, strict: at equality neither atom is
    attended, no dot is made and the call fails with "No molecular dots generated"; one step inside both spheres are sampled.
    same_*: atoms 0 and 1 of molecule 0 (r = 2.5: bridge distance 8.4) at d = 8.0 and one step outside; atom 2 gives atom 0 a second
    neighbour (a pair alone ends in the num_neighbors <= 1 break) and atom 3 of molecule 1 makes all of them attended.  The map is
    inclusive (d^2 <= sep^2): at equality the pair (0, 1) has its toroidal dots; outside, 0 and 1 are left with one neighbour each (atom
    2), every pair ends in the break and there is no toroidal dot at all."""
    c = {}
    for name, d in (("other_at", 8.0), ("other_inside", float(np.nextafter(8.0, 0.0)))):
        c[name] = (_inp([[0.0, 0.0, 0.0], [0.0, 0.0, d]], [2.5, 2.5], [0, 1]), dict(DEFAULTS))
    for name, d in (("same_at", 8.0), ("same_outside", float(np.nextafter(8.0, np.inf)))):
        c[name] = (_inp([[0.0, 0.0, 0.0], [d, 0.0, 0.0], [4.0, 4.5, 0.25], [4.0, -1.0, 5.5]], [2.5, 2.5, 1.5, 1.8], [0, 0, 0, 1]), dict(DEFAULTS))
    return c


# ---- wide boxes
TRIM_EDGE = 1.5  # the trimmed-dot cells' requested edge (sc.inl launch_sc)


def cell_dims(inp: dict, st: dict, edge_req: float):
    """(nx, ny, nz), capped: the cell counts per axis of a device cell list with requested edge edge_req, and whether the 128-per-axis
    cap decided the edge."""
    pad = float(inp["r"].max()) + 2.0 * st["rp"] + 1.0
    lo = [float(inp[a].min()) - pad for a in "xyz"]
    hi = [float(inp[a].max()) + pad for a in "xyz"]
    ext = max(h - l for h, l in zip(hi, lo))
    edge = max(edge_req, ext / 128.0)
    inv = 1.0 / edge
    return tuple(int((h - l) * inv) + 1 for h, l in zip(hi, lo)), edge > edge_req


def open_edge(st: dict) -> float:
    return st["band"] * (1.0 + 1e-9) + 1e-9


WIDE_FAR = {"three_level": 150.0, "capped": 230.0}  # the far atom's offset from the halves' centre along (1, 1, 1)


def wide_box(which: str | None) -> tuple:
    """The 600-atom halves, plus (which != None) one atom of molecule 0 appended last, far along the diagonal.  It is Far and has no
    neighbour, so no dot or probe changes; only the box does.  three_level: every axis of the padded box is between 152 and 192 A, the
    1.5 A cell lists of the open and the trimmed dots have more than 1024^2 cells and the cap is off; capped: the box is wider than 192 A."""
    h = halves(600)
    if which is not None:
        c = np.round(np.array([h[a].mean() for a in "xyz"])) + WIDE_FAR[which]
        for k, a in enumerate("xyz"):
            h[a] = np.append(h[a], c[k])
        h["r"] = np.append(h["r"], 1.8)
        h["mol"] = np.append(h["mol"], np.uint8(0))
    return h, dict(DEFAULTS)


# ---- settings one at a time, and one combined off-default point
def settings_sweep() -> dict:
    # (450 atoms at band = 0.2 and 300 at the combined point, where almost every buried dot is trimmed and the restatement's scans grow)
    c = {f"{k}{v}": (halves(n), dict(DEFAULTS, **{k: v})) for k, v, n in (("band", 0.2, 450), ("band", 3.0, 600), ("w", 2.0, 600), ("rp", 0.5, 600),
                                                                       ("rp", 3.0, 600))}
    c["combined"] = (halves(300), dict(rp=2.2, density=22.0, band=2.0, sep=9.0, w=0.8))
    return c


# ---- equal d^2 in a neighbour list
def d2_ties(order_seed: int | None = None) -> tuple:
    """Atoms in mirror pairs (+-x, y, z) about atoms on the plane x = 0, on a quarter-Angstrom lattice (dyadic: every d^2 is exact).  An
    atom on the plane has its own pair as its two nearest neighbours, at bit-equal d^2 -- neighbour 0, the north pole of its contact dots,
    is decided by the index half of the sort alone -- and sees every other pair at equal d^2 too; the atoms of a pair see the partners of
    every other pair at equal d^2 crosswise.  Which partner has the higher index alternates, and the partner at -x lies in the cell below
    the plane's (the atoms' cells are 8 A wide and start 6.3 A below the lowest x), so the higher index is now in the lower cell, now in
    the atom's own.  The lattice jitter keeps atoms off common axes; the shear y += z / 8, equal for both partners, keeps the ties.
    order_seed permutes the atoms, with the original index carried as the serial."""
    rng = np.random.default_rng(0x7135)
    xyz, mol = [], []
    q = lambda lo, hi: float(rng.integers(int(lo * 4), int(hi * 4) + 1)) / 4.0
    k = 0
    for m, z0, sgn in ((0, -1.75, -1.0), (1, 2.25, 1.0)):
        for layer in range(2):
            for iy in range(4):
                y, z = 4.5 * iy + q(-0.25, 0.25), z0 + sgn * 4.0 * layer + q(-0.25, 0.25)
                xyz.append([0.0, y, z]); mol.append(m)
                xm = 1.5 + 0.25 * ((3 * iy + 5 * layer + 2 * m) % 7)
                a = [xm, y + 1.0 + q(0.0, 0.25), z + sgn * q(0.25, 0.75)]
                pair = [a, [-xm, a[1], a[2]]]
                if k % 2:
                    pair.reverse()
                k += 1
                xyz += pair; mol += [m, m]
    xyz = np.array(xyz)
    xyz[:, 1] += xyz[:, 2] / 8.0
    n = len(xyz)
    r = np.where(np.arange(n) % 3 == 0, 1.9, 1.7)  # (mirror partners share a radius)
    serial = np.arange(n, dtype=np.int64)
    mol = np.array(mol)
    if order_seed is not None:
        p = np.random.default_rng(order_seed).permutation(n)
        xyz, r, serial, mol = xyz[p], r[p], serial[p], mol[p]
    return _inp(xyz, r, mol, serial), dict(DEFAULTS)
