"""ctypes loader of tests/sc_restatement.c (the sequential C restatement of shape complementarity) and the test-side inputs for it.

The radii here come from tests/golden/sc_radii.csv through this module's own wildcard_match, not through the product's table; the
element fallback is the pdbtbx van-der-Waals radius (arp_params.vdw_radius).  compile() builds the C file with the host compiler into a
directory the caller owns (pytest's tmp_path), so the product's build is not involved."""
from __future__ import annotations

import ctypes as C
import csv
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SRC = HERE / "sc_restatement.c"
RADII_CSV = HERE / "golden" / "sc_radii.csv"
SETTINGS = dict(rp=1.7, density=15.0, band=1.5, sep=8.0, w=0.5)  # settings.rs defaults
ERRORS = {1: "No atoms defined", 2: "No atoms for chain group 1", 3: "No molecular dots generated", 4: "Overlapping atoms detected",
          5: "Sampling limit exceeded"}

# the quirk branches the restatement counts (scr_branches): surface_generator.rs :494-496 return / :497 continue, :620-627, :418-422, :654-685
BRANCHES = ("wedge_return", "wedge_continue", "ring_return", "lonely_break", "far_j_arc")
# how far a run went into the paths of tests/sc_edge_cases.py (scr_reach): the largest latitude count of a contact atom / a concave probe
# that emitted a dot, neighbour-list entries with the d^2 of the entry before them, triplet candidates k that only "k is not in j's map"
# rejected (d_jk < e_j + e_k), ordered same-molecule pairs inside the bridge distance that only d^2 <= sep^2 rejected, concave dots of a
# probe's latitudes 64 and up
REACH = ("max_lat_contact", "max_lat_probe", "d2_ties", "kmap_rejects", "sep_rejects", "probe_dots_past_64")


class ScrResults(C.Structure):
    _fields_ = [(k, C.c_int64 * 2) for k in ("n_atoms", "n_buried_atoms", "n_far_atoms", "n_all_dots", "n_trimmed_dots")] + \
               [(k, C.c_double * 2) for k in ("trimmed_area", "d_mean", "d_median", "s_mean", "s_median")] + \
               [(k, C.c_int64) for k in ("n_convex", "n_toroidal", "n_concave", "n_probes")] + \
               [(k, C.c_double) for k in ("sc", "distance", "area")] + [(k, C.c_int32) for k in ("err", "err_i", "err_j")]


def compile(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libsc_restatement.so"
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"], check=True)
    L = C.CDLL(str(so))
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    L.scr_run.restype = vp
    L.scr_run.argtypes = [C.c_int, dp, dp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)] + [C.c_double] * 5 + [C.POINTER(ScrResults)]
    L.scr_n_dots.restype = C.c_int64
    L.scr_n_dots.argtypes = [vp, C.c_int]
    L.scr_dots.argtypes = [vp, C.c_int, dp, dp, dp, C.POINTER(C.c_int32), dp, dp]
    L.scr_n_probes.restype = C.c_int64
    L.scr_n_probes.argtypes = [vp]
    L.scr_probes.argtypes = [vp, C.POINTER(C.c_int32), dp, dp]
    L.scr_branches.argtypes = [vp, C.POINTER(C.c_int64)]
    L.scr_reach.argtypes = [vp, C.POINTER(C.c_int64)]
    L.scr_free.argtypes = [vp]
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def run(L, x, y, z, r, mol, serial=None, **settings) -> dict:
    """Results as a dict (err: 0 or an ERRORS key), the per-surface dots (xyz, normal, area, flags, nn_dist, score), the probes, the
    branch counts (BRANCHES) and the reach counters (REACH)."""
    st = dict(SETTINGS, **settings)
    n = len(x)
    x, y, z, r = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, z, r))
    mol = np.ascontiguousarray(mol, dtype=np.int32)
    serial = np.arange(n, dtype=np.int64) if serial is None else np.ascontiguousarray(serial, dtype=np.int64)
    res = ScrResults()
    h = L.scr_run(n, _p(x, C.c_double), _p(y, C.c_double), _p(z, C.c_double), _p(r, C.c_double), _p(mol, C.c_int32), _p(serial, C.c_int64),
                  st["rp"], st["density"], st["band"], st["sep"], st["w"], C.byref(res))
    try:
        out = {k: (list(getattr(res, k)) if isinstance(getattr(res, k), C.Array) else getattr(res, k)) for k, _ in ScrResults._fields_}
        out["dots"] = []
        for s in range(2):
            m = L.scr_n_dots(h, s)
            d = {"xyz": np.zeros((m, 3)), "normal": np.zeros((m, 3)), "area": np.zeros(m), "flags": np.zeros(m, np.int32),
                 "nn_dist": np.zeros(m), "score": np.zeros(m)}
            if m:
                L.scr_dots(h, s, _p(d["xyz"], C.c_double), _p(d["normal"], C.c_double), _p(d["area"], C.c_double), _p(d["flags"], C.c_int32),
                           _p(d["nn_dist"], C.c_double), _p(d["score"], C.c_double))
            out["dots"].append(d)
        m = L.scr_n_probes(h)
        pa, ph, pp = np.zeros((m, 3), np.int32), np.zeros(m), np.zeros((m, 3))
        if m:
            L.scr_probes(h, _p(pa, C.c_int32), _p(ph, C.c_double), _p(pp, C.c_double))
        out["probes"] = {"atoms": pa, "height": ph, "point": pp}
        br = np.zeros(len(BRANCHES), dtype=np.int64)
        L.scr_branches(h, _p(br, C.c_int64))
        out["branches"] = dict(zip(BRANCHES, br.tolist()))
        rc = np.zeros(len(REACH), dtype=np.int64)
        L.scr_reach(h, _p(rc, C.c_int64))
        out["reach"] = dict(zip(REACH, rc.tolist()))
    finally:
        L.scr_free(h)
    return out


def radius_table():
    with open(RADII_CSV) as f:
        return [(row["residue"], row["atom"], float(row["radius"])) for row in csv.DictReader(f)]


def wildcard_match(query: str, pattern: str) -> bool:
    """atomic_radii.rs:413-440, restated: trailing spaces trimmed from both; a leading '*' matches anything; a '*' at position p matches
    when the first p characters agree; otherwise the strings must be equal."""
    q, p = query.rstrip(" "), pattern.rstrip(" ")
    if p.startswith("*"):
        return True
    star = p.find("*")
    if star >= 0:
        return len(q) >= star and q[:star] == p[:star]
    return q == p


def sc_radius(resn: str, atomn: str, element_vdw: float, table=None) -> float:
    for res, atom, rad in table or radius_table():
        if wildcard_match(resn, res) and wildcard_match(atomn, atom):
            return rad
    return element_vdw if element_vdw > 0 else 0.0


def structure_inputs(structure, groups: str, model_num: int = 0) -> dict:
    """Raw arrays of the SC selection (the product's host selection, arpeggia_amd.sc_select) with this module's radii."""
    import arpeggia_amd as aa
    from arpeggia_amd import _lib

    atoms, mol = aa.sc_select(structure, groups, model_num)
    soa = structure.soa()
    resn, name, elem = (structure.strings(c)[atoms] for c in ("resn", "atomn", "element"))
    p = aa.default_params()
    table = radius_table()
    r = np.array([sc_radius(rn.decode(), an.decode(), p.vdw_radius[_lib.lib.arp_element_class(e)], table) for rn, an, e in zip(resn, name, elem)])
    return {"x": soa["x"][atoms], "y": soa["y"][atoms], "z": soa["z"][atoms], "r": r, "mol": mol,
            "serial": np.asarray(structure.ints("atomi"), dtype=np.int64)[atoms], "atoms": atoms}
