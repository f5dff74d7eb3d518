"""Torsion angles (arp_torsions) without a device: the host twin arp_torsions_host against pinned values of the two files, the numpy restatement of
tests/torsion_cases.py and built torsions; undefined torsions, transitions, the mirror image and rigid motion; torsion_select; the input checks of arp_torsions
(ctx == NULL); the table; the twin alone under the address and undefined-behaviour sanitizers in a stand-alone program.  Expected values never come from the
call under test: they are pinned, derived in the docstrings, or come from the restatement.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import subprocess
from fractions import Fraction
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import torsion_cases as tc
import trajectory_shapes as ts
from arpeggia_amd import _lib
from arpeggia_amd import build as arp_build

ROOT = Path(__file__).resolve().parent.parent
PHI, PSI, OMEGA, CHI1, CHI2, CHI3, CHI4, CHI5 = range(8)


@lru_cache(maxsize=None)
def from_file(name: str):
    """(structure, selection, xyz [N, 3]) of a test file through the product's loader and torsion_select."""
    s = aa.Structure.load(str(tc.DATA / name))
    sel = aa.torsion_select(s)
    soa = s.soa()
    n = aa.api._topology_atoms(s)
    xyz = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1).astype(np.float64)
    return s, sel, xyz


def twin(quad_xyz, B=36, pairs=None, G=0):
    return aa.torsions_host(quad_xyz, pairs, G, B)


def bits(angles) -> np.ndarray:
    return np.ascontiguousarray(angles, "<f4").view("<u4")


def test_exported():
    assert {"arp_torsions", "arp_torsions_host"} <= set(_lib.EXPORTS)
    header = (ROOT / "include" / "arpeggia_amd.h").read_text()
    assert "arp_status arp_torsions(" in header and "arp_status arp_torsions_host(" in header
    for name in ("torsion_select", "get_torsions", "torsions", "torsions_host", "torsion_table", "TORSION_KINDS", "TORSION_COLUMNS"):
        assert hasattr(aa, name), name
    assert aa.TORSION_KINDS == ["phi", "psi", "omega", "chi1", "chi2", "chi3", "chi4", "chi5"]


# ---- pinned values --------------------------------------------------------------------------------------------------------------------------------------------------
def test_ubq_pinned():
    s, sel, xyz = from_file("1ubq.pdb")
    assert len(sel["quads"]) == 386 and np.bincount(sel["kind"], minlength=8).tolist() == [75, 75, 75, 68, 54, 24, 11, 4]
    assert len(sel["pairs"]) == 74 and np.bincount(sel["rama_class"], minlength=4).tolist() == [64, 5, 3, 2]
    res = twin(tc.gather(xyz[None], sel["quads"]), 36, sel["pairs"], 4)
    angle = {(int(r), int(k)): float(a) for r, k, a in zip(sel["row"], sel["kind"], res["angles"][0])}
    want = {(0, PSI): 149.6288, (0, OMEGA): 178.3074, (0, CHI1): 80.3654, (0, CHI2): -172.1514, (0, CHI3): 177.5043, (1, PHI): -91.0202, (1, PSI): 138.2641}
    for key, a in want.items():
        assert abs(angle[key] - a) <= 1e-3, (key, angle[key], a)     # 10^-3 degrees: the precision of the file's coordinates propagated
    assert (0, PHI) not in angle
    om = sel["kind"] == OMEGA
    assert (res["cossin"][0, om, 0] < 0).all() and (res["states"][0, om] == 2).all()            # no cis omega, all 75 trans
    assert res["state_counts"][sel["kind"] == PHI][:, 1:].sum(0).tolist() == [6, 10, 59]
    assert res["state_counts"][sel["kind"] == CHI1][:, 1:].sum(0).tolist() == [11, 20, 37]
    assert int(res["hist2"].sum()) == 74 and res["hist2"].sum((1, 2)).tolist() == [64, 5, 3, 2]


def test_bft_pinned():
    s, sel, xyz = from_file("6bft.pdb")
    assert len(sel["quads"]) == 4984 and np.bincount(sel["kind"], minlength=8).tolist() == [1045, 1045, 1045, 924, 600, 211, 86, 28]
    assert len(sel["pairs"]) == 1035 and np.bincount(sel["rama_class"], minlength=4).tolist() == [844, 73, 60, 58]
    res = twin(tc.gather(xyz[None], sel["quads"]))
    om = np.flatnonzero(sel["kind"] == OMEGA)
    cis = om[res["cossin"][0, om, 0] > 0]
    assert sel["row"][cis].tolist() == [6, 93, 139, 363, 365, 444, 531, 577, 800, 802, 903, 996]


def test_margins_of_the_files():
    """The margins of the two files as DESIGN.md section 3.24 records them (two digits), by the restatement."""
    for name, edge, c, s_ in (("1ubq.pdb", 3.8e-4, 6.5e-4, 9.5e-4), ("6bft.pdb", 8.4e-4, 7.6e-5, 1.5e-5)):
        _, sel, xyz = from_file(name)
        q = tc.gather(xyz[None], sel["quads"])
        a = tc.restate(q)["a"]
        got = min(tc.edge_margin(a, 36), tc.edge_margin(a, 72))
        m = tc.decision_margins(q)
        assert abs(got - edge) <= 0.05 * edge and abs(m["c"] - c) <= 0.05 * c and abs(m["s"] - s_) <= 0.05 * s_, (name, got, m)


# ---- the twin against the restatement -------------------------------------------------------------------------------------------------------------------------------
def assert_twin_is_restatement(q, B, pairs=None, G=0):
    res, r = twin(q, B, pairs, G), tc.restate(q, B)
    assert np.array_equal(res["states"], r["state"])
    assert np.array_equal(np.isnan(res["angles"]), ~r["defined"]) and (bits(res["angles"])[~r["defined"]] == tc.NAN_BITS).all()
    assert np.abs(res["cossin"][..., 0] - r["c"]).max() <= 1e-12 and np.abs(res["cossin"][..., 1] - r["s"]).max() <= 1e-12
    ok = r["defined"]
    assert (np.abs(res["angles"][ok].astype(np.float64) - r["a"][ok]) <= 1e-12 + np.spacing(np.abs(r["a"][ok]).astype(np.float32)) / 2).all()   # (one rounding to f32)
    want = tc.over_frames(r, B, pairs, G)
    for key in ("n_defined", "state_counts", "n_transitions", "hist") + (("hist2",) if G else ()):
        assert np.array_equal(res[key], want[key]), key
    F = q.shape[0]
    assert (np.abs(res["sums"] - want["sums"]) <= F * 2.0 ** -52 * np.maximum(want["n_defined"], 1)[:, None]).all()
    return res


@pytest.mark.parametrize("name", ["1ubq.pdb", "6bft.pdb"])
def test_twin_against_the_restatement(name):
    _, sel, xyz = from_file(name)
    c = tc.case(name, xyz[None], sel["quads"], (36, 72))
    for B in c["bins"]:
        assert_twin_is_restatement(tc.gather(c["frames"], c["quads"]), B, sel["pairs"], 4)


def test_twin_against_the_restatement_on_jittered_frames():
    _, sel, xyz = from_file("1ubq.pdb")
    c = tc.jittered("1ubq_jitter9", xyz, sel["quads"], 9, 21, (36, 360))
    for B in c["bins"]:
        res = assert_twin_is_restatement(tc.gather(c["frames"], c["quads"]), B, sel["pairs"], 4)
    assert res["n_transitions"].sum() > 0 and len(tc.SKIPPED_SEEDS) <= 1


# ---- built torsions -------------------------------------------------------------------------------------------------------------------------------------------------
def test_built_angles():
    """p0 = (1,0,0), p1 = 0, p2 = (0,0,1), p3 = (u, v, 1): b1 = (-1,0,0), b2 = (0,0,1), b3 = (u,v,0); n1 = (0,1,0), n2 = (-v,u,0); x = u, y = 1 * v, every
    product exact.  So with integer p3: trans (-1,0,1) has x = -1, y = 0: a = atan2(0, -1) = +180, c = -1: state t, bin 0 (180 + 180 = 360 = B w wraps);
    cis (1,0,1): a = 0, state g+ (s = 0 >= 0), bin B / 2; (0,1,1): +90, g+; (0,-1,1): -90, g-."""
    B = 36
    q = np.array([tc.built_integer(t) for t in (180, 0, 90, -90)])[None]
    res = twin(q, B)
    assert res["angles"][0].tolist() == [180.0, 0.0, 90.0, -90.0]
    assert res["states"][0].tolist() == [2, 1, 1, 3]
    assert res["cossin"][0].tolist() == [[-1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]
    assert [int(np.flatnonzero(row)[0]) for row in res["hist"][:2]] == [0, B // 2]      # (+-90 sit on an edge of the 10-degree bins: not asserted)
    for theta, state in ((60.0, 1), (-60.0, 3), (120.5, 2), (-120.5, 2), (119.5, 1), (-119.5, 3)):
        r = twin(tc.built(theta)[None, None], B)
        assert abs(float(r["angles"][0, 0]) - theta) <= 1e-5 and r["states"][0, 0] == state, theta
    grid = np.arange(-179, 181)
    r = twin(np.array([tc.built(float(t)) for t in grid])[None], 360)
    assert np.abs(r["angles"][0].astype(np.float64) - grid).max() <= 2e-5      # (f32 of 180 has a spacing of 1.5e-5)
    # half a degree off the 1-degree grid, no angle is near an edge: theta + 0.5 lands in bin floor(theta + 180.5)
    r = twin(np.array([tc.built(t + 0.5) for t in grid[:-1]])[None], 360)
    assert np.array_equal(np.argmax(r["hist"], 1), grid[:-1] + 180)


def exact_c(u: float, v: float) -> float:
    """c of the construction with p3 = (u, v, 1) in exact rational arithmetic, rounded where the definition rounds: h = sqrt(fl(fl(u u) + fl(v v))), c = fl(u / h)."""
    z = float(Fraction(float(Fraction(u) ** 2)) + Fraction(float(Fraction(v) ** 2)))
    h = math.sqrt(z)
    lo, hi = Fraction(np.nextafter(h, 0.0)), Fraction(np.nextafter(h, np.inf))
    assert ((Fraction(h) + lo) / 2) ** 2 <= Fraction(z) <= ((Fraction(h) + hi) / 2) ** 2     # h is the correctly rounded root
    return float(Fraction(u) / Fraction(h))


def test_theta_120_is_decided_by_c():
    """The construction at theta = 120 degrees has u = fl(cos(fl(2 pi / 3))).  fl(2 pi / 3) lies below 2 pi / 3, the cosine falls there, so u is above -1/2 by a
    few units of 2^-53; v = fl(sin ..) makes u u + v v round to 1 or its neighbour, and c = fl(u / h) stays above -0.5: NOT t.  s > 0: the state is g+, the
    well [0, 120).  With u = -0.5 exactly and v = fl(sqrt(0.75)), h is 1 or 1 + 2^-52 and c is -0.5 or just above: decided by the exact arithmetic below."""
    t = np.radians(120.0)
    u, v = float(np.cos(t)), float(np.sin(t))
    assert u > -0.5
    c = exact_c(u, v)
    assert c > -0.5
    r = twin(tc.built(120.0)[None, None])
    assert r["cossin"][0, 0, 0] == c and r["states"][0, 0] == 1
    q = tc.built(0.0)
    q[3] = (-0.5, math.sqrt(0.75), 1.0)
    c = exact_c(-0.5, math.sqrt(0.75))
    r = twin(q[None, None])
    assert r["cossin"][0, 0, 0] == c and r["states"][0, 0] == (2 if c <= -0.5 else 1)


def test_undefined_torsions():
    """p0 = p1 (b1 = 0: n1 = 0, x = 0, y = |b2| * 0 = 0, h = 0) and a collinear triple (n1 = 0 and b1 . n2 = 0 exactly in integers) are undefined: NaN bits,
    (0, 0), state 0, in no count but state_counts[0], in no histogram, and no transition across them: frames g+ . g+ and g+ . t of torsion 0 and 1 with the
    undefined frame between count 0 transitions, although 1 -> 2 would be one."""
    same = tc.built(65.0)
    same[0] = same[1]
    gp, t = tc.built(65.0), tc.built(175.0)
    q = np.array([[gp, gp, tc.COLLINEAR], [same, tc.COLLINEAR, tc.COLLINEAR], [gp, t, tc.COLLINEAR]])     # [F = 3, D = 3]
    pairs = np.array([[0, 1, 0], [0, 2, 0]], "<u4")
    res = twin(q, 36, pairs, 1)
    assert res["states"].tolist() == [[1, 1, 0], [0, 0, 0], [1, 2, 0]]
    assert (bits(res["angles"])[res["states"] == 0] == tc.NAN_BITS).all() and (res["cossin"][res["states"] == 0] == 0).all()
    assert res["n_defined"].tolist() == [2, 2, 0] and res["state_counts"].tolist() == [[1, 2, 0, 0], [1, 1, 1, 0], [3, 0, 0, 0]]
    assert res["n_transitions"].tolist() == [0, 0, 0]
    assert res["hist"].sum(1).tolist() == [2, 2, 0] and int(res["hist2"].sum()) == 2          # pair (0, 1): frames 0 and 2; pair (0, 2): never
    assert np.isnan(res["mean"][2]) and np.isnan(res["resultant"][2]) and abs(res["mean"][0] - 65.0) <= 1e-12
    assert_twin_is_restatement(q, 36, pairs, 1)


def test_transitions_of_a_state_sequence():
    """1 1 3 0 3 2 2 1: 1 -> 3, (3 -> 0 and 0 -> 3 do not count), 3 -> 2, 2 -> 1 = 3 transitions; without its last frame, 1 1 3 0 3 2 2, two."""
    seq = [1, 1, 3, 0, 3, 2, 2, 1]
    res = twin(tc.state_frames(seq)[:, None])
    assert res["states"][:, 0].tolist() == seq and res["n_transitions"].tolist() == [3]
    assert twin(tc.state_frames(seq[:-1])[:, None])["n_transitions"].tolist() == [2]
    assert twin(tc.state_frames([2])[:, None])["n_transitions"].tolist() == [0]


def test_mirror_image():
    """x -> -x negates every angle (c is kept, s changes sign, both exactly: every product changes sign or keeps it): g+ and g- swap, and away from the edges bin k
    becomes bin B - 1 - k."""
    _, sel, xyz = from_file("1ubq.pdb")
    c = tc.jittered("1ubq_mirror", xyz, sel["quads"], 5, 31)
    q = tc.gather(c["frames"], c["quads"])
    a, b = twin(q), twin(tc.mirrored(q))
    assert np.array_equal(a["cossin"][..., 0], b["cossin"][..., 0]) and np.array_equal(a["cossin"][..., 1], -b["cossin"][..., 1])
    assert np.array_equal(a["angles"], -b["angles"])
    assert np.array_equal(a["state_counts"][:, [0, 3, 2, 1]], b["state_counts"]) and np.array_equal(a["n_transitions"], b["n_transitions"])
    assert np.array_equal(a["hist"][:, ::-1], b["hist"])


def test_rigid_tumble_keeps_states_and_bins():
    _, sel, xyz = from_file("1ubq.pdb")
    frames = ts.tumble(xyz, 5, 4)
    assert tc.clear(frames, sel["quads"], (36,))
    res = twin(tc.gather(frames, sel["quads"]))
    assert (res["states"] == res["states"][:1]).all() and res["n_transitions"].sum() == 0
    assert (res["hist"].max(1) == 5).all()
    assert np.abs(res["angles"] - res["angles"][:1]).max() <= 4 * 2.0 ** -17      # 2 ulp of f32 at 180 (2^-16): the f64 angles move by 1e-12


# ---- torsion_select -------------------------------------------------------------------------------------------------------------------------------------------------
def peptide(residues: list, gap_after=None, chain_of=None) -> list:
    """Atoms (trajectory_shapes.records) of a built backbone with CB and, for SER, OG; gap_after: the residue whose bond to the next is stretched to 3 A."""
    import dssp_cases as dc

    bb = dc.backbone([(-60.0, -45.0)] * len(residues))
    atoms = []
    shift = np.zeros(3)
    for r, resn in enumerate(residues):
        chain = chain_of(r) if chain_of else "A"
        n, ca, c, o = bb[r] + shift
        members = [("N", "N", n), ("CA", "C", ca), ("C", "C", c), ("O", "O", o)]
        if resn != "GLY":
            cb = dc.place(c, n, ca, 1.53, 110.5, -122.5)
            members.append(("CB", "C", cb))
            if resn == "SER":
                members.append(("OG", "O", dc.place(n, ca, cb, 1.42, 111.0, 60.0)))
        atoms += [(resn, name, elem, chain, r + 1, tuple(p)) for name, elem, p in members]
        if gap_after == r:      # |C[r] - N[r + 1]| becomes 3 A, along the bond
            d = bb[r + 1][0] - bb[r][2]
            shift = shift + d / np.linalg.norm(d) * (3.0 - np.linalg.norm(d))
    return atoms


def kinds_by_row(sel: dict) -> dict:
    out = {}
    for r, k in zip(sel["row"], sel["kind"]):
        out.setdefault(int(r), []).append(aa.TORSION_KINDS[int(k)])
    return out


def test_torsion_select_links_and_missing_atoms():
    res = ["ALA", "SER", "GLY", "SER", "PRO", "ALA"]
    s = aa.Structure.from_records(ts.records(peptide(res)))
    sel = aa.torsion_select(s)
    full = ["phi", "psi", "omega"]
    assert kinds_by_row(sel) == {0: ["psi", "omega"], 1: full + ["chi1"], 2: full, 3: full + ["chi1"], 4: full, 5: ["phi"]}   # (the built PRO has no CG: no chi)
    assert sel["n_rows"] == 6 and sel["rama_class"].tolist() == [0, 1, 3, 2]        # rows 1 .. 4: SER, GLY, SER before PRO, PRO
    assert sel["pairs"][:, 2].tolist() == sel["rama_class"].tolist()
    names = s.strings("atomn")
    q = sel["quads"][(sel["row"] == 1) & (sel["kind"] == CHI1)][0]
    assert [names[k].decode() for k in q] == ["N", "CA", "CB", "OG"]
    q = sel["quads"][(sel["row"] == 1) & (sel["kind"] == PHI)][0]
    assert [names[k].decode() for k in q] == ["C", "N", "CA", "C"] and s.ints("resi")[q].tolist() == [1, 2, 2, 2]
    q = sel["quads"][(sel["row"] == 1) & (sel["kind"] == OMEGA)][0]
    assert [names[k].decode() for k in q] == ["CA", "C", "N", "CA"] and s.ints("resi")[q].tolist() == [2, 2, 3, 3]
    # a missing CB drops chi1 only; the residue stays
    atoms = [a for a in peptide(res) if not (a[4] == 2 and a[1] == "CB")]
    sel2 = aa.torsion_select(aa.Structure.from_records(ts.records(atoms)))
    assert kinds_by_row(sel2)[1] == full and sel2["n_rows"] == 6
    # kinds
    only = aa.torsion_select(s, kinds=("phi", "chi1"))
    assert set(only["kind"].tolist()) == {PHI, CHI1} and len(only["pairs"]) == 0
    assert len(aa.torsion_select(s, kinds="omega")["quads"]) == 5
    with pytest.raises(ValueError, match="Invalid torsion kind"):
        aa.torsion_select(s, kinds=("chi9",))


def test_torsion_select_breaks():
    res = ["ALA"] * 6
    # a 3 A gap after residue 3: |C - N| > 2.5, no psi / omega of 3 and no phi of 4
    gap = aa.torsion_select(aa.Structure.from_records(ts.records(peptide(res, gap_after=2))))
    assert kinds_by_row(gap) == {0: ["psi", "omega"], 1: ["phi", "psi", "omega"], 2: ["phi"], 3: ["psi", "omega"], 4: ["phi", "psi", "omega"], 5: ["phi"]}
    # a chain change at the same place, the geometry unbroken
    two = aa.Structure.from_records(ts.records(peptide(res, chain_of=lambda r: "A" if r < 3 else "B")))
    assert kinds_by_row(aa.torsion_select(two)) == kinds_by_row(gap)
    assert kinds_by_row(aa.torsion_select(two, "B")) == {0: ["psi", "omega"], 1: ["phi", "psi", "omega"], 2: ["phi"]}
    # HOH between two residues is not a residue of the selection: the link is by geometry
    atoms = peptide(res)
    at = next(k for k, a in enumerate(atoms) if a[4] == 4)
    atoms.insert(at, ("HOH", "O", "O", "A", 100, (50.0, 50.0, 50.0)))
    assert kinds_by_row(aa.torsion_select(aa.Structure.from_records(ts.records(atoms))))[3] == ["phi", "psi", "omega"]


def test_torsion_select_takes_the_first_altloc():
    """Two CB of residue 2 (a second conformer behind the first): chi1 is built on the first, and nothing else changes."""
    res = ["ALA", "SER", "ALA"]
    atoms = peptide(res)
    at = next(k for k, a in enumerate(atoms) if a[4] == 2 and a[1] == "CB")
    atoms.insert(at + 1, ("SER", "CB", "C", "A", 2, (9.0, 9.0, 9.0)))
    sel = aa.torsion_select(aa.Structure.from_records(ts.records(atoms)))
    ref = aa.torsion_select(aa.Structure.from_records(ts.records(peptide(res))))
    assert np.array_equal(sel["kind"], ref["kind"]) and np.array_equal(sel["row"], ref["row"])
    q = sel["quads"][(sel["row"] == 1) & (sel["kind"] == CHI1)][0]
    assert q[2] == at and (sel["quads"] != at + 1).all()


# ---- the input checks of arp_torsions, ctx == NULL -------------------------------------------------------------------------------------------------------------------
def check_call(structure, frames, quads, bins=36, pairs=None, G=0, hist=True, hist2=False, n_tors=None):
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    quads = np.ascontiguousarray(quads, "<u4").reshape(-1, 4)
    pr = np.zeros((0, 3), "<u4") if pairs is None else np.ascontiguousarray(pairs, "<u4").reshape(-1, 3)
    keep = (quads if quads.size else np.zeros(4, "<u4")), (pr if pr.size else np.zeros(3, "<u4")), np.zeros(1, "<u4")
    n_frames, ptr = (0, None) if frames is None else (len(frames), np.ascontiguousarray(frames, "<f8").ctypes.data_as(dp))
    some = keep[2].ctypes.data_as(u32p)   # (a non-null pointer: with ctx == NULL no output is written)
    st = _lib.lib.arp_torsions(None, structure._h, n_frames, ptr, keep[0].ctypes.data_as(u32p), len(quads) if n_tors is None else n_tors, bins, keep[1].ctypes.data_as(u32p),
                               len(pr), G, None, None, None, None, None, None, None, some if hist else None, some if hist2 else None)
    return st, _lib.lib.arp_last_error().decode()


@pytest.fixture(scope="module")
def small():
    s = aa.Structure.from_records(ts.records(peptide(["ALA"] * 4)))
    sel = aa.torsion_select(s)
    soa = s.soa()
    return s, sel, np.stack([soa["x"], soa["y"], soa["z"]], 1)[None].astype(np.float64)


def test_checks_pass(small):
    s, sel, frames = small
    assert check_call(s, frames, sel["quads"], 36, sel["pairs"], 4, hist2=True)[0] == _lib.ARP_OK
    assert check_call(s, None, sel["quads"], 0, hist=False)[0] == _lib.ARP_OK


def test_check_no_torsions(small):
    s, sel, frames = small
    assert check_call(s, frames, sel["quads"][:0]) == (_lib.ARP_ERR_BAD_INPUT, "torsions: no torsions (n_tors == 0)")


def test_check_atom_index(small):
    s, sel, frames = small
    bad = sel["quads"].copy()
    bad[2, 3] = 20
    assert check_call(s, frames, bad) == (_lib.ARP_ERR_BAD_INPUT, "torsions: quads[2][3] = 20 is not an atom of the topology (20 atoms)")


def test_check_bins(small):
    s, sel, frames = small
    assert check_call(s, frames, sel["quads"], 361) == (_lib.ARP_ERR_BAD_INPUT, "torsions: n_bins = 361, at most 360 are supported")
    assert check_call(s, frames, sel["quads"], 360)[0] == _lib.ARP_OK


def test_check_histogram_without_bins(small):
    s, sel, frames = small
    want = (_lib.ARP_ERR_BAD_INPUT, "torsions: a histogram is asked for with n_bins == 0")
    assert check_call(s, frames, sel["quads"], 0, hist=True) == want
    assert check_call(s, frames, sel["quads"], 0, sel["pairs"], 4, hist=False, hist2=True) == want


def test_check_hist2_without_groups_or_pairs(small):
    s, sel, frames = small
    assert check_call(s, frames, sel["quads"], 36, sel["pairs"], 0, hist2=True) == (_lib.ARP_ERR_BAD_INPUT, "torsions: hist2 is asked for with n_groups == 0 and n_pairs == 2")
    assert check_call(s, frames, sel["quads"], 36, None, 4, hist2=True) == (_lib.ARP_ERR_BAD_INPUT, "torsions: hist2 is asked for with n_groups == 4 and n_pairs == 0")


def test_check_pairs(small):
    s, sel, frames = small
    D = len(sel["quads"])
    bad = sel["pairs"].copy()
    bad[1, 1] = D
    assert check_call(s, frames, sel["quads"], 36, bad, 4, hist2=True) == (_lib.ARP_ERR_BAD_INPUT, f"torsions: pairs[1][1] = {D} is not a torsion ({D} torsions)")
    bad = sel["pairs"].copy()
    bad[0, 2] = 4
    assert check_call(s, frames, sel["quads"], 36, bad, 4, hist2=True) == (_lib.ARP_ERR_BAD_INPUT, "torsions: pairs[0][2] = 4 is not a group (4 groups)")


def test_check_frames_and_capacity(small):
    s, sel, frames = small
    assert check_call(s, frames[:0], sel["quads"]) == (_lib.ARP_ERR_BAD_INPUT, "contact frequencies: at least one frame is needed")
    nan = np.repeat(frames, 2, 0)
    nan[1, 7, 1] = np.nan
    assert check_call(s, nan, sel["quads"]) == (_lib.ARP_ERR_BAD_INPUT, "contact frequencies: non-finite coordinate in frame 1, atom 7")
    with pytest.raises(aa.ArpeggiaError, match=r"torsions: frames must have shape \[F, 20, 3\]"):
        aa.api._torsions(None, s, frames[:, :-1], "", ("phi",), 36, "class", True, False, False)
    with pytest.raises(ValueError, match="Invalid rama"):
        aa.api._torsions(None, s, frames, "", ("phi",), 36, "pair", True, False, False)
    aa.debug_set("rmsd_cap_bytes", 64)
    try:
        st, msg = check_call(s, frames, sel["quads"])
        assert st == _lib.ARP_ERR_CAPACITY and msg.startswith("torsions: the states of 1 frames (F) x 9 torsions (D)") and msg.endswith("the limit is 64 (rmsd_cap_bytes)")
    finally:
        aa.debug_set("rmsd_cap_bytes", 0)
    with pytest.raises(aa.ArpeggiaError, match="torsions: at least one frame is needed"):
        aa.torsions_host(np.zeros((0, 1, 4, 3)))
    with pytest.raises(aa.ArpeggiaError, match="torsions: non-finite coordinate in frame 0, torsion 0"):
        aa.torsions_host(np.full((1, 1, 4, 3), np.inf))


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_table_and_statistics():
    s, sel, xyz = from_file("1ubq.pdb")
    frames = np.stack([xyz, xyz, xyz])
    res = twin(tc.gather(frames, sel["quads"]))
    res.update({k: sel[k] for k in ("kind", "residue", "row")})
    r = tc.restate(tc.gather(xyz[None], sel["quads"]))
    assert np.abs(res["mean"] - r["a"][0]).max() <= 1e-9 and np.abs(res["resultant"] - 1.0).max() <= 1e-15 and res["circ_std"].max() <= 1e-5
    assert res["state_fraction"].dtype == np.float32 and (res["state_fraction"].sum(1) == 1.0).all()
    table = aa.torsion_table(s, res)
    cols = {name: table[name].to_list() if hasattr(table[name], "to_list") else table[name].to_pylist() for name in aa.TORSION_COLUMNS}
    assert list(cols) == aa.TORSION_COLUMNS and len(cols["chain"]) == 386
    assert cols["torsion"][:6] == ["psi", "omega", "chi1", "chi2", "chi3", "phi"] and cols["resn"][:6] == ["MET"] * 5 + ["GLN"] and cols["resi"][:6] == [1] * 5 + [2]
    assert cols["n_defined"][0] == 3 and cols["n_transitions"][0] == 0 and abs(cols["mean"][0] - 149.6288) <= 1e-3
    assert (cols["frac_gplus"][2], cols["frac_trans"][2], cols["frac_gminus"][2]) == (1.0, 0.0, 0.0)     # chi1 of MET 1 = 80.4: g+
    # two opposite angles: the resultant vanishes, the circular standard deviation grows without bound
    res2 = twin(np.array([tc.built(90.0), tc.built(-90.0)])[:, None])
    assert res2["resultant"][0] <= 1e-15 and res2["circ_std"][0] > 400.0


# ---- the twin alone under the sanitizers ------------------------------------------------------------------------------------------------------------------------------
def test_twin_under_sanitizers(tmp_path):
    """The host twin alone in a stand-alone program (tests/torsion_host), built with -fsanitize=address,undefined, on D = 1 .. 5 and the whole of 1ubq with its
    74 pairs: every buffer is a heap block of exactly its size, so an access out of range ends the program.  It prints the states, checked against the restatement."""
    _, sel, xyz = from_file("1ubq.pdb")
    q = tc.gather(np.stack([xyz, ts.jitter(xyz, 1, 3)[0]]), sel["quads"])
    cases = [(q[:, :n], np.zeros((0, 3), "<u4"), 0) for n in (1, 2, 3, 4, 5)] + [(q, sel["pairs"], 4)]
    blob = struct.pack("<Q", len(cases))
    for x, pairs, G in cases:
        blob += struct.pack("<QQIQI", x.shape[0], x.shape[1], 36, len(pairs), G) + np.ascontiguousarray(x, "<f8").tobytes() + np.ascontiguousarray(pairs, "<u4").tobytes()
    (tmp_path / "cases.bin").write_bytes(blob)
    prog = tmp_path / "torsion_host_main"
    subprocess.run([arp_build.hipcc(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "torsion_host" / "torsion_host_main.cpp"), "-o", str(prog)], check=True, capture_output=True)
    run = subprocess.run([str(prog), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    want = []
    for x, pairs, G in cases:
        r = tc.restate(x, 36)
        want += ["".join(str(int(v)) for v in row) for row in r["state"]]
        want.append(f"hist2 {len(pairs) * 2 if G else 0}")
    assert run.stdout.split("\n")[:-1] == want
