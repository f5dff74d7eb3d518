"""CPU restatement of the atom-SASA contract (include/arpeggia_amd.h "atom SASA", DESIGN.md "Atom SASA") in numpy + scipy, and of the SAP
score built on it (src/sap.rs:137-340) from the oracle's sap_weight / sap_neighbor_sum.  No product imports: the GPU tests compare the engine
with this, so it must not share code with it.

The rule, written out in f64 from the f32 inputs: point k of atom i is buried iff some other atom j has
    d^2 = tx*tx + ty*ty + tz*tz  <  R_j * R_j,   t = (c_i - c_j) + s_k * R_i  per axis,
numpy evaluating every operation in IEEE f64 left to right without contraction -- the same roundings as the kernel's explicit ones.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

K4PI = 4.0 * 3.141592653589793


def sphere_points(n: int) -> np.ndarray:
    """Golden spiral: t = k/n, theta = acos(1 - 2t), phi = (2 pi golden) k, in f64, rounded to f32 -> n x 3."""
    k = np.arange(n, dtype=np.float64)
    golden = (1.0 + np.sqrt(5.0)) / 2.0
    t = k / n
    theta = np.arccos(1.0 - 2.0 * t)
    phi = (2.0 * 3.141592653589793 * golden) * k
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1).astype(np.float32)


def atom_counts(x, y, z, R, sphere, homes=None, chunk_pairs=20000):
    """Accessible point count of every atom in `homes` (default: all), against all atoms.  x, y, z are rounded to f32 here; R is f32
    (radius + probe); sphere is the f32 n x 3 table the engine uses (arp_sasa_sphere_points)."""
    c = np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64)], axis=1).astype(np.float32).astype(np.float64)
    R = np.asarray(R, np.float32)
    n = len(c)
    homes = np.arange(n) if homes is None else np.asarray(homes)
    npts = len(sphere)
    s = sphere.astype(np.float64)
    Rd = R.astype(np.float64)
    rmax = float(R.max()) if n else 0.0
    tree = cKDTree(c)
    # candidates: |c_i - c_j| <= R_i + R_max (a burier has |c_i - c_j| < R_i |s| + R_j); the exact test below decides
    nb = tree.query_ball_point(c[homes], r=(Rd[homes] + rmax) * (1 + 1e-6) + 1e-9)
    hi = np.repeat(np.arange(len(homes)), [len(v) for v in nb])
    hj = np.concatenate([np.asarray(v, dtype=np.int64) for v in nb]) if len(homes) else np.zeros(0, np.int64)
    keep = homes[hi] != hj  # self excluded by index
    hi, hj = hi[keep], hj[keep]
    buried = np.zeros((len(homes), npts), dtype=bool)
    for a in range(0, len(hi), chunk_pairs):
        pi, pj = hi[a:a + chunk_pairs], hj[a:a + chunk_pairs]
        i = homes[pi]
        ri = Rd[i][:, None]
        tx = (c[i, 0] - c[pj, 0])[:, None] + s[None, :, 0] * ri
        ty = (c[i, 1] - c[pj, 1])[:, None] + s[None, :, 1] * ri
        tz = (c[i, 2] - c[pj, 2])[:, None] + s[None, :, 2] * ri
        d2 = tx * tx + ty * ty + tz * tz
        hit = d2 < (Rd[pj] * Rd[pj])[:, None]
        np.logical_or.at(buried, pi, hit)
    return (npts - buried.sum(axis=1)).astype(np.int32)


def sasa_from_counts(R, counts, n_points) -> np.ndarray:
    """f32(((4 pi R) R count) / n) in f64."""
    Rd = np.asarray(R, np.float32).astype(np.float64)
    return ((((K4PI * Rd) * Rd) * np.asarray(counts, np.float64)) / float(n_points)).astype(np.float32)


BACKBONE = [b"N", b"CA", b"C", b"O", b"OXT"]


def per_atom_sap(rows: dict, nb: dict, sap_radius: float, sap_weight, sap_neighbor_sum):
    """sap.rs:137-259 restated on plain columns.
    rows: the atom-SASA rows (serial i32, sasa f32, resn bytes), sorted by serial;
    nb: the neighbour set (x, y, z f64, serial i32, name bytes, resn bytes) = the structure after chain filter, H and solvent removal, all models;
    all_non_backbone_serials: see the caller.  Returns the score of every neighbour-set atom (0 for backbone atoms)."""
    sasa_of = {}
    for sr, a in zip(rows["serial"], rows["sasa"]):
        sasa_of[int(sr)] = float(a)
    resn_with_row = set(rows["resn"].tolist())
    side = ~np.isin(nb["name"], BACKBONE)
    w = np.zeros(len(nb["x"]), dtype=np.float32)
    for k, (sr, rn) in enumerate(zip(nb["serial"], nb["resn"])):
        if int(sr) in sasa_of and rn in resn_with_row:
            w[k] = sap_weight(rn.decode(), sasa_of[int(sr)])
    return sap_neighbor_sum(nb["x"], nb["y"], nb["z"], side, w, sap_radius), side


def residue_group_by(chain, resn, resi, insertion, sc_sasa, sap, max_sc_asa: dict):
    """sap.rs:308-337: sap_score > 0, group by (chain, resn, resi, insertion), sums (f64, rounded to f32), sort by chain, resi, insertion."""
    groups = {}
    for c, rn, ri, ic, a, s in zip(chain, resn, resi, insertion, sc_sasa, sap):
        if not s > 0.0:
            continue
        g = groups.setdefault((c, rn, int(ri), ic), [0.0, 0.0])
        g[0] += float(a)
        g[1] += float(s)
    keys = sorted(groups, key=lambda k: (k[0], k[2], k[3]))
    sc = np.array([groups[k][0] for k in keys], np.float64).astype(np.float32)
    sp = np.array([groups[k][1] for k in keys], np.float64).astype(np.float32)
    mx = np.array([max_sc_asa[k[1]] for k in keys], np.float32)
    rel = np.clip(sc / mx, np.float32(0), np.float32(1)).astype(np.float32) if keys else np.zeros(0, np.float32)
    return keys, sc, sp, mx, rel
