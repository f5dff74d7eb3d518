"""A third, plain statement of the per-pair contact rules, and inputs that sit on their decision boundaries.  TEST INFRASTRUCTURE ONLY.

The product decides in squared-distance space against bounds the host precomputes (engine.cpp bound_lt / bound_le) and the oracle takes the
square root and compares; neither is pinned where a pair lies within a few ulps of a threshold.  This module restates the rules once more, in
Python floats and the reference's operation order (pdbtbx Atom::distance / angle / dihedral; vdw.rs, hbond.rs, ionic.rs, hydrophobic.rs,
complex.rs:189-299), and builds motif sets whose pairs sit at -4 .. +4 coordinate ulps around every bound.  It imports neither the product
nor the oracle: the radius table and the atom-class predicates below are its own (predicates only for the residues the motifs use:
EDGE_RESIDUES; callers restrict other inputs to pairs of those residues).

  contacts(atoms, groups, vdw_comp, cutoff)  -> {(i, j): (kind bits, f64 distance, s)}   all candidate pairs, ligand atom first
  classify(atoms, res_atoms, i, j, vdw_comp) -> kind bits of one candidate pair (complex.rs:217-296)
  gen_edges(family, vdw_comp, place)         -> EdgeSet: synth-style records + the restatement's atoms + the sweeps
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

INTERACTIONS = [
    "StericClash", "CovalentBond", "Disulfide", "VanDerWaalsContact", "IonicBond", "HydrogenBond",
    "WeakHydrogenBond", "PolarContact", "WeakPolarContact", "IonicRepulsion", "SaltBridge",
    "PiDisplacedStacking", "PiTStacking", "PiSandwichStacking", "PiParallelInPlaneStacking",
    "PiTiltedStacking", "PiLStacking", "CationPi", "HydrophobicContact",
]
BIT = {name: 1 << k for k, name in enumerate(INTERACTIONS)}

# pdbtbx 0.12 Element::atomic_radius: (covalent_single: Pyykko & Atsumi 2009, van_der_waals: Alvarez 2013), for the sixteen element classes
# of the product's default parameters
RADII = {
    "C": (0.75, 1.77), "N": (0.71, 1.66), "O": (0.63, 1.50), "S": (1.03, 1.89), "H": (0.32, 1.20), "P": (1.11, 1.90),
    "SE": (1.16, 1.82), "F": (0.64, 1.46), "CL": (0.99, 1.82), "BR": (1.14, 1.86), "I": (1.33, 2.04), "NA": (1.55, 2.50),
    "MG": (1.39, 2.51), "K": (1.96, 2.73), "CA": (1.71, 2.62), "ZN": (1.18, 2.39),
}
RAD2DEG = 180.0 / math.pi  # f64::to_degrees
VDW_COMPS = (0.1, 0.0, 0.25, 1.0, -0.1, -0.6)
CUTOFFS = (0.5, 3.0, 4.0, 6.5, 12.0)

# ---------------------------------------------------------------------------------------------- atom classes (the motifs' residues only)
EDGE_RESIDUES = {"GLY", "ALA", "LYS", "ASP", "GLU", "CYS"}


def is_acceptor(resn, name):  # hbond.rs:137-157
    if name in ("O", "OXT") and resn != "HOH":
        return True
    return (resn, name) in {("ASP", "OD1"), ("ASP", "OD2"), ("GLU", "OE1"), ("GLU", "OE2"), ("CYS", "SG")}


def is_donor(resn, name):  # hbond.rs:160-178
    return name == "N" or (resn, name) in {("LYS", "NZ"), ("CYS", "SG")}


def is_weak_donor(name, elem):  # hbond.rs:204-207
    return elem == "C" and name != "C"


def is_pos(resn, name):  # ionic.rs:84-91
    return (resn, name) == ("LYS", "NZ")


def is_neg(resn, name):  # ionic.rs:94-99
    return (resn, name) in {("ASP", "OD1"), ("ASP", "OD2"), ("GLU", "OE1"), ("GLU", "OE2")}


def is_hydrophobic(res_resn, name):  # hydrophobic.rs:27-45
    if name == "CB" and res_resn != "SER":
        return True
    return (res_resn, name) in {("GLU", "CG"), ("LYS", "CG"), ("LYS", "CD")}


# ---------------------------------------------------------------------------------------------- geometry (pdbtbx, no FMA: Python floats)
def sq(a, b):
    dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    return dx * dx + dy * dy + dz * dz


def dist(a, b):
    return math.sqrt(sq(a, b))


def _acos(q):
    return math.acos(q) if -1.0 <= q <= 1.0 else math.nan  # (Rust f64::acos: NaN outside [-1, 1] and for NaN)


def angle(a, b, c):
    """Angle at b between b->a and b->c, degrees."""
    ba = (a[0] - b[0], a[1] - b[1], a[2] - b[2])
    bc = (c[0] - b[0], c[1] - b[1], c[2] - b[2])
    nba = math.sqrt(0.0 + ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2])
    nbc = math.sqrt(0.0 + bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2])
    dot = 0.0 + ba[0] * bc[0] + ba[1] * bc[1] + ba[2] * bc[2]
    den = nba * nbc
    return _acos(dot / den if den != 0.0 else math.nan) * RAD2DEG


def dihedral(a, b, c, d):
    ba = (a[0] - b[0], a[1] - b[1], a[2] - b[2])
    bc = (c[0] - b[0], c[1] - b[1], c[2] - b[2])
    cb = (b[0] - c[0], b[1] - c[1], b[2] - c[2])
    cd = (d[0] - c[0], d[1] - c[1], d[2] - c[2])
    n1 = (ba[1] * bc[2] - ba[2] * bc[1], ba[2] * bc[0] - ba[0] * bc[2], ba[0] * bc[1] - ba[1] * bc[0])
    n2 = (cb[1] * cd[2] - cb[2] * cd[1], cb[2] * cd[0] - cb[0] * cd[2], cb[0] * cd[1] - cb[1] * cd[0])
    a1 = math.sqrt(0.0 + n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2])
    a2 = math.sqrt(0.0 + n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2])
    dot = 0.0 + n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2]
    den = a1 * a2
    return _acos(dot / den if den != 0.0 else math.nan) * RAD2DEG


# ---------------------------------------------------------------------------------------------- the rules
@dataclass
class Atom:
    xyz: tuple
    name: str
    resn: str       # conformer name (hbond.rs, ionic.rs)
    res_resn: str   # residue name (hydrophobic.rs, vdw.rs)
    elem: str
    chain: str
    model: int
    res: int        # residue id: atoms with the same id are one residue
    res_ord: int    # position of the residue in its chain (complex.rs:411-440)


def _hbond_like(atoms, res_atoms, d, a, c, min_angle, strong, polar):
    """hbond.rs:36-63 / 80-107: some hydrogen of the donor's residue within reach of the acceptor at the angle -> strong, else polar at 3.5."""
    da = dist(atoms[d].xyz, atoms[a].xyz)
    if da <= 4.0:
        lim = RADII["H"][1] + RADII[atoms[a].elem][1] + c
        for h in res_atoms[atoms[d].res]:
            if atoms[h].elem != "H":
                continue
            if dist(atoms[h].xyz, atoms[a].xyz) <= lim and angle(atoms[d].xyz, atoms[h].xyz, atoms[a].xyz) >= min_angle:
                return strong
    return polar if da <= 3.5 else None


def _disulfide(atoms, res_atoms, i, j):
    """vdw.rs:46-80: both CYS SG; |dihedral(CB1, SG1, SG2, CB2)| in [60, 120]."""
    e1, e2 = atoms[i], atoms[j]
    if not (e1.res_resn == e2.res_resn == "CYS" and e1.name == e2.name == "SG"):
        return False
    first = lambda r, nm: next(k for k in res_atoms[r] if atoms[k].name == nm)
    q = [first(e1.res, "CB"), first(e1.res, "SG"), first(e2.res, "SG"), first(e2.res, "CB")]
    return 60.0 <= abs(dihedral(*(atoms[k].xyz for k in q))) <= 120.0


def classify(atoms, res_atoms, i, j, c):
    """complex.rs:217-296 for the candidate pair (i ligand, j receptor): the set rows as bits."""
    e1, e2 = atoms[i], atoms[j]
    d = dist(e1.xyz, e2.xyz)
    sum_cov = RADII[e1.elem][0] + RADII[e2.elem][0]
    sum_vdw = RADII[e1.elem][1] + RADII[e2.elem][1]
    kind = 0
    if d < sum_cov - c:
        return BIT["StericClash"]
    if d < sum_cov + c:
        kind |= BIT["Disulfide"] if _disulfide(atoms, res_atoms, i, j) else BIT["CovalentBond"]
    elif d < sum_vdw + c:
        kind |= BIT["VanDerWaalsContact"]
    ionic = ((is_pos(e1.resn, e1.name) and is_neg(e2.resn, e2.name)) or (is_pos(e2.resn, e2.name) and is_neg(e1.resn, e1.name))) and d <= 4.0
    hb = None
    if is_donor(e1.resn, e1.name) and is_acceptor(e2.resn, e2.name):
        hb = _hbond_like(atoms, res_atoms, i, j, c, 90.0, "HydrogenBond", "PolarContact")
    elif is_donor(e2.resn, e2.name) and is_acceptor(e1.resn, e1.name):
        hb = _hbond_like(atoms, res_atoms, j, i, c, 90.0, "HydrogenBond", "PolarContact")
    if ionic:
        kind |= BIT["SaltBridge"] if hb == "HydrogenBond" else BIT["IonicBond"]
    elif hb:
        kind |= BIT[hb]
    weak = None
    if is_weak_donor(e1.name, e1.elem) and is_acceptor(e2.resn, e2.name):
        weak = _hbond_like(atoms, res_atoms, i, j, c, 130.0, "WeakHydrogenBond", "WeakPolarContact")
    elif is_weak_donor(e2.name, e2.elem) and is_acceptor(e1.resn, e1.name):
        weak = _hbond_like(atoms, res_atoms, j, i, c, 130.0, "WeakHydrogenBond", "WeakPolarContact")
    if weak:
        kind |= BIT[weak]
    both_pos = is_pos(e1.resn, e1.name) and is_pos(e2.resn, e2.name)
    both_neg = is_neg(e1.resn, e1.name) and is_neg(e2.resn, e2.name)
    if (both_pos or both_neg) and d <= 4.0:
        kind |= BIT["IonicRepulsion"]
    if is_hydrophobic(e1.res_resn, e1.name) and is_hydrophobic(e2.res_resn, e2.name) and d <= 4.5:
        kind |= BIT["HydrophobicContact"]
    return kind


def parse_groups(chains, groups):
    """utils.rs:71-115: "lig/rec", comma lists; an empty side is the complement of the other, both empty = every chain on both sides."""
    lig_s, rec_s = groups.split("/")[:2]
    lig = {c for c in lig_s.split(",") if c}
    rec = {c for c in rec_s.split(",") if c}
    if not lig and not rec:
        return set(chains), set(chains)
    if not lig:
        lig = set(chains) - rec
    elif not rec:
        rec = set(chains) - lig
    return lig, rec


def should_compare(e1, e2, lig, rec):
    """complex.rs:76-131 with symmetric = true (e1 in the ligand set, e2 in the receptor set)."""
    if e1.elem == "H" or e2.elem == "H" or e1.model != e2.model:
        return False
    l1, l2, c1, c2 = e1.chain in lig, e2.chain in lig, e1.chain in rec, e2.chain in rec
    if not ((l1 and c2) or (l2 and c1)):
        return False
    if e1.chain == e2.chain:
        return e2.res_ord > 1 and e1.res_ord < e2.res_ord - 1
    return not (c1 and c2 and l1 and l2 and e1.chain > e2.chain)


def residue_index(atoms):
    res_atoms = {}
    for k, a in enumerate(atoms):
        res_atoms.setdefault(a.res, []).append(k)
    return res_atoms


def contacts(atoms, groups="/", vdw_comp=0.1, cutoff=6.5):
    """get_atomic_contacts (complex.rs:189-299): every ligand atom x (not H) against every receptor atom y with d^2 <= cutoff^2 (rstar,
    inclusive) that should_compare admits.  {(x, y): (kind bits, f64 distance, d^2)}.  A k-d tree only proposes pairs (with slack); the
    decision is the plain one above."""
    from scipy.spatial import cKDTree

    lig, rec = parse_groups(sorted({a.chain for a in atoms}), groups)
    res_atoms = residue_index(atoms)
    r2 = cutoff * cutoff
    heavy = [k for k, a in enumerate(atoms) if a.elem != "H"]
    out = {}
    if not heavy:
        return out
    xyz = np.array([atoms[k].xyz for k in heavy])
    tree = cKDTree(xyz)
    for p, q in tree.query_pairs(cutoff * (1 + 1e-9) + 1e-9, output_type="ndarray"):
        for x, y in ((heavy[p], heavy[q]), (heavy[q], heavy[p])):
            ex, ey = atoms[x], atoms[y]
            if ex.chain not in lig or ey.chain not in rec:
                continue
            s = sq(ex.xyz, ey.xyz)
            if s <= r2 and should_compare(ex, ey, lig, rec):
                out[(x, y)] = (classify(atoms, res_atoms, x, y, vdw_comp), math.sqrt(s), s)
    return out


# ---------------------------------------------------------------------------------------------- float steps
def _ord(v):
    i = int(np.float64(v).view(np.int64))
    return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)


def _unord(i):
    return float(np.int64(i if i >= 0 else (-i) | -0x8000000000000000).view(np.float64))


def step(v, k):
    """v moved by k ulps (across zero as well)."""
    return _unord(_ord(v) + k)


def find_flip(pred, lo, hi):
    """Bisection over the doubles between lo and hi (pred(lo) != pred(hi)): the first v with pred(v) == pred(hi)."""
    a, b = _ord(lo), _ord(hi)
    pa = pred(lo)
    assert pa != pred(hi), "the bracket does not straddle the boundary"
    while abs(b - a) > 1:
        m = (a + b) // 2
        if pred(_unord(m)) == pa:
            a = m
        else:
            b = m
    return _unord(b)


# ---------------------------------------------------------------------------------------------- motif sets
EDGE_ELEMS = [e for e in RADII if e != "H"]   # hydrogens never pair (complex.rs:76-79): their bounds are unreachable
DIRS = {"axis": (1.0, 0.0, 0.0), "face": (1.0, 1.0, 0.0), "body": (1.0, 1.0, 1.0)}
OFFSETS = range(-4, 5)
SPACING = 20.0      # lattice step: wider than the largest motif (< 6.5 A) plus the largest cutoff
FAR = 9999.0
MIDPOINT_OFFSETS = (0, 1, -1, 2, -2, 3, -3, 10, -10, 100, -100, 1000, -1000, 2040, -2040, 2047, -2047, 2048, -2048, 2049, -2049, 2056, -2056,
                    2500, -2500, 3000, -3000)


@dataclass
class Sweep:
    label: str
    pairs: list          # (x, y) per offset: the designated pair, ligand atom first
    bound: float = 0.0   # the threshold the sweep straddles (distance space; 0 for angle / midpoint sweeps)
    live: bool = True    # False: the bound is shadowed by another (vdw.rs first match with c <= 0) -- both outcomes are not expected
    kind: str = "rule"   # "rule" (kind bits), "cutoff" (candidate or not), "f32" (the f32 distance rounds down or up)


@dataclass
class EdgeSet:
    family: str
    vdw_comp: float
    place: str
    atoms: list = field(default_factory=list)
    sweeps: list = field(default_factory=list)

    def records(self) -> dict:
        """synth-style records (tests/synth.py) in chain order, so that file order is hierarchy order."""
        n = len(self.atoms)
        resi = {}
        cols = {"x": [], "y": [], "z": [], "name": [], "resn": [], "chain": [], "resi": [], "element": []}
        for a in self.atoms:
            cols["x"].append(a.xyz[0]); cols["y"].append(a.xyz[1]); cols["z"].append(a.xyz[2])
            cols["name"].append(a.name.encode()); cols["resn"].append(a.resn.encode()); cols["chain"].append(a.chain.encode())
            cols["resi"].append(resi.setdefault(a.res, a.res_ord + 1)); cols["element"].append(a.elem.encode())
        return {
            "x": np.array(cols["x"], dtype="<f8"), "y": np.array(cols["y"], dtype="<f8"), "z": np.array(cols["z"], dtype="<f8"),
            "occupancy": np.ones(n), "serial": np.arange(1, n + 1, dtype=np.int32), "resi": np.array(cols["resi"], dtype=np.int32),
            "model_serial": np.zeros(n, dtype=np.int32), "name": np.array(cols["name"], dtype="S8"), "resn": np.array(cols["resn"], dtype="S8"),
            "chain": np.array(cols["chain"], dtype="S8"), "altloc": np.zeros(n, dtype="S4"), "icode": np.zeros(n, dtype="S4"),
            "element": np.array(cols["element"], dtype="S4"),
        }


class _Builder:
    """Motifs on a lattice.  Residues are collected per chain and numbered in order, the atoms are emitted chain by chain."""

    def __init__(self, origin, n_slots):
        self.origin = origin
        side = max(1, math.ceil(n_slots ** (1.0 / 3.0)))
        self.side = side
        self.slot = 0
        self.chains = {}   # chain -> list of residues (list of (name, resn, elem, xyz))
        self.handles = []  # (chain, residue index, atom index in residue) per atom added, resolved in finish()

    def point(self):
        k = self.slot
        self.slot += 1
        i, j, l = k // (self.side * self.side), (k // self.side) % self.side, k % self.side  # x slowest: the first motifs share x = origin x
        o = self.origin
        return (o[0] + SPACING * i, o[1] + SPACING * j, o[2] + SPACING * l)

    def residue(self, chain, resn, atoms):
        """atoms: [(name, elem, xyz)] -> handles of the atoms."""
        res = self.chains.setdefault(chain, [])
        res.append((resn, atoms))
        return [(chain, len(res) - 1, k) for k in range(len(atoms))]

    def finish(self, es: EdgeSet):
        index, rid = {}, 0
        for chain in sorted(self.chains):
            for r, (resn, atoms) in enumerate(self.chains[chain]):
                for k, (name, elem, xyz) in enumerate(atoms):
                    index[(chain, r, k)] = len(es.atoms)
                    es.atoms.append(Atom(tuple(float(v) for v in xyz), name, resn, resn, elem, chain, 0, rid, r))
                rid += 1
        for sw in es.sweeps:
            sw.pairs = [(index[a], index[b]) for a, b in sw.pairs]
        return es


def _inert(elem):
    """(name, residue) of an atom of this element that no class predicate matches."""
    return (elem + "Q", "GLY")


def _unit(v):
    n = math.sqrt(sum(x * x for x in v))
    return tuple(x / n for x in v)


def _pair_sweep(b, es, label, elems, names, resns, T, decide, direction, kind="rule", live=True):
    """Two atoms in two chains at distance ~T along `direction`; the x coordinate of the second one stepped by ulps around the point where
    decide(s) flips."""
    u = _unit(DIRS[direction])
    handles = []
    for off in OFFSETS:
        P = b.point()
        Q = [P[0] + T * u[0], P[1] + T * u[1], P[2] + T * u[2]]
        pred = lambda x: decide(sq(P, (x, Q[1], Q[2])))
        x0 = find_flip(pred, Q[0] - 1e-6 * (1.0 + abs(Q[0])), Q[0] + 1e-6 * (1.0 + abs(Q[0])))
        Q[0] = step(x0, off)
        h1 = b.residue("A", resns[0], [(names[0], elems[0], P)])
        h2 = b.residue("B", resns[1], [(names[1], elems[1], Q)])
        handles.append((h1[0], h2[0]))
    es.sweeps.append(Sweep(label, handles, T, live, kind))


def _radii_family(b, es, c):
    for ia, ea in enumerate(EDGE_ELEMS):
        for eb in EDGE_ELEMS[ia:]:
            (ca, va), (cb, vb) = RADII[ea], RADII[eb]
            sum_cov, sum_vdw = ca + cb, va + vb
            t_clash, t_cov, t_vdw = sum_cov - c, sum_cov + c, sum_vdw + c
            na, ra = _inert(ea)
            nb, rb = _inert(eb)
            for what, T, live in (("clash", t_clash, True), ("cov", t_cov, t_cov > t_clash), ("vdw", t_vdw, t_vdw > max(t_clash, t_cov))):
                for dname in DIRS:
                    _pair_sweep(b, es, f"{what} {ea}-{eb} {dname}", (ea, eb), (na, nb), (ra, rb), T, lambda s, T=T: math.sqrt(s) < T, dname, live=live)


def _fixed_bounds(b, es, c):
    le = lambda T: (lambda s: math.sqrt(s) <= T)
    cases = [  # (label, bound, (name, resn, elem) x 2)
        ("polar 3.5 N..O", 3.5, ("N", "GLY", "N"), ("O", "GLY", "O")),
        ("weak polar 3.5 CB..O", 3.5, ("CB", "ALA", "C"), ("O", "GLY", "O")),
        ("ionic 4.0 NZ..OD1", 4.0, ("NZ", "LYS", "N"), ("OD1", "ASP", "O")),
        ("repulsion 4.0 OD1..OE1", 4.0, ("OD1", "ASP", "O"), ("OE1", "GLU", "O")),
        ("hydrophobic 4.5 CB..CB", 4.5, ("CB", "ALA", "C"), ("CB", "ALA", "C")),
    ]
    for label, T, a1, a2 in cases:
        for dname in DIRS:
            _pair_sweep(b, es, f"{label} {dname}", (a1[2], a2[2]), (a1[0], a2[0]), (a1[1], a2[1]), T, le(T), dname)
    for cut in CUTOFFS:
        r2 = cut * cut
        for dname in DIRS:
            _pair_sweep(b, es, f"cutoff {cut} {dname}", ("C", "C"), ("CQ", "CQ"), ("GLY", "GLY"), cut, lambda s, r2=r2: s <= r2, dname, kind="cutoff")


def _hacc_sweeps(b, es, c):
    """The H..acceptor bound (hbond.rs:54,98): donor, its hydrogen and the acceptor, the H..A distance swept at a comfortable angle."""
    donors = (("strong", ("N", "GLY", "N"), 90.0), ("weak", ("CB", "ALA", "C"), 130.0))
    acceptors = (("O", ("O", "GLY", "O")), ("S", ("SG", "CYS", "S")))
    for dl, (dn, dr, de), _ in donors:
        for al, (an, ar, ae) in acceptors:
            T = RADII["H"][1] + RADII[ae][1] + c
            for dname in DIRS:
                u = _unit(DIRS[dname])
                handles = []
                for off in OFFSETS:
                    P = b.point()
                    Hp = [P[0] + T * u[0], P[1] + T * u[1], P[2] + T * u[2]]
                    x0 = find_flip(lambda x: math.sqrt(sq(P, (x, Hp[1], Hp[2]))) <= T, Hp[0] - 1e-6 * (1 + abs(Hp[0])), Hp[0] + 1e-6 * (1 + abs(Hp[0])))
                    Hp[0] = step(x0, off)
                    # the donor beyond H, 10 degrees off the H..A line, so that D..A stays within 4.0 A and the angle far above 130 degrees
                    dd = max(0.1, min(0.9, 3.9 - T))
                    w = _unit((u[1], -u[0], 0.0))  # u x z
                    D = tuple(Hp[k] + dd * (math.cos(0.17) * u[k] + math.sin(0.17) * w[k]) for k in range(3))
                    hd = b.residue("A", dr, [(dn, de, D), ("H", "H", tuple(Hp))])
                    ha = b.residue("B", ar, [(an, ae, P)])
                    handles.append((hd[0], ha[0]))
                es.sweeps.append(Sweep(f"H..acceptor {dl} {al} {dname}", handles, T, T + dd < 3.999))


def _angle_sweeps(b, es, c):
    """Donor-H-acceptor angles across 90 (strong) and 130 degrees (weak): the acceptor's largest-moving coordinate stepped by ulps."""
    r = 1.9 if c >= -0.2 else 1.6  # H..A within the H..acceptor bound for every compensation (1.2 + 1.5 - 0.6 = 2.1)
    frames = [((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0)), ((1.0, 1.0, 0.0), (0.0, 0.0, 1.0)), ((1.0, 1.0, 1.0), (1.0, -1.0, 0.0))]
    for strength, (dn, dr, de), theta in (("strong", ("N", "GLY", "N"), 90.0), ("weak", ("CB", "ALA", "C"), 130.0)):
        for fi, (u, w) in enumerate(frames):
            u, w = _unit(u), _unit(w)
            k = max(range(3), key=lambda q: abs(u[q]))
            handles = []
            for off in OFFSETS:
                P = b.point()
                D = tuple(P[q] + 1.5 * u[q] for q in range(3))  # (D..A stays above the N..O clash bound for every compensation)
                t = math.radians(theta)
                A = [P[q] + r * (math.cos(t) * u[q] + math.sin(t) * w[q]) for q in range(3)]

                def pred(v, A=A, P=P, D=D):
                    B = list(A); B[k] = v
                    return angle(D, P, B) >= theta

                span = 1e-6 * (1 + abs(A[k]))
                v0 = find_flip(pred, A[k] + span * (1 if u[k] > 0 else -1), A[k] - span * (1 if u[k] > 0 else -1))
                if theta == 90.0 and fi < 2 and off == 0:
                    v0 = P[k]  # the dot product exactly 0: acos(0) * 180 / pi == 90.0 exactly, a hydrogen bond (>= 90)
                    B = list(A); B[k] = v0
                    assert angle(D, P, B) == 90.0
                A[k] = step(v0, off) if not (theta == 90.0 and fi < 2 and off == 0) else v0
                hd = b.residue("A", dr, [(dn, de, D), ("H", "H", P)])
                ha = b.residue("B", "GLY", [("O", "O", tuple(A))])
                handles.append((hd[0], ha[0]))
            es.sweeps.append(Sweep(f"angle {theta:g} {strength} frame {fi}", handles))


def _dihedral_sweeps(b, es, c):
    """CB-SG-SG-CB across 60 and 120 degrees (vdw.rs:78), the SG pair inside the covalent band (for c > 0)."""
    dss = 2.06 + (c / 2.0 if c > 0 else 0.0)
    for phi, inside_above in ((60.0, True), (120.0, False)):
        for g in range(2):
            handles = []
            for off in OFFSETS:
                P = b.point()
                S1, S2 = P, (P[0] + dss, P[1], P[2])
                CB1 = (P[0] - 0.6, P[1] + 1.7, P[2])
                t = math.radians(phi)
                CB2 = [S2[0] + 0.6, S2[1] + 1.7 * math.cos(t), S2[2] + 1.7 * math.sin(t)]
                q = 2 if g == 0 else 1

                def pred(v, CB2=CB2, q=q):
                    X = list(CB2); X[q] = v
                    dh = abs(dihedral(CB1, S1, S2, X))
                    return dh >= 60.0 if inside_above else dh <= 120.0

                span = 1e-6 * (1 + abs(CB2[q]))
                CB2[q] = step(find_flip(pred, CB2[q] - span, CB2[q] + span), off)
                h1 = b.residue("A", "CYS", [("CB", "C", CB1), ("SG", "S", S1)])
                h2 = b.residue("B", "CYS", [("SG", "S", S2), ("CB", "C", tuple(CB2))])
                handles.append((h1[1], h2[0]))
            es.sweeps.append(Sweep(f"dihedral {phi:g} geometry {g}", handles, 0.0, c > 0))


def _f32_midpoints(b, es):
    """Distances on an f32 rounding midpoint (ties round to even) and +-1 .. +-3000 f64 ulps around it: dx fixed on or below the midpoint,
    a small dy lifts s to the wanted ulp."""
    for f in (np.float32(0.7), np.float32(1.3), np.float32(2.2), np.float32(3.3), np.float32(3.7), np.float32(5.9)):
        for up_even in (False, True):
            lo32 = f if (int(f.view(np.uint32)) & 1) == (0 if not up_even else 1) else np.nextafter(f, np.float32(10))
            m = (float(lo32) + float(np.nextafter(lo32, np.float32(10)))) / 2.0
            u = math.ulp(m)
            handles = []
            for off in MIDPOINT_OFFSETS:
                P = b.point()
                target = m + off * u
                x2 = P[0] + m  # (exact: the lattice points have few significant bits)
                while x2 - P[0] > target:  # dx at or below the target
                    x2 = step(x2, -1)
                dxr = x2 - P[0]
                rest = target * target - dxr * dxr
                dy = math.sqrt(rest) if rest > 0 else 0.0
                Q = (x2, P[1] + dy, P[2])
                h1 = b.residue("A", "GLY", [("CQ", "C", P)])
                h2 = b.residue("B", "GLY", [("CQ", "C", Q)])
                handles.append((h1[0], h2[0]))
            es.sweeps.append(Sweep(f"f32 midpoint {m!r}", handles, m, True, "f32"))
    # coincident and near-coincident pairs
    for dx in (0.0, 1e-20, 1e-9):
        P = b.point()
        b.residue("A", "GLY", [("CQ", "C", P)])
        b.residue("B", "GLY", [("CQ", "C", (P[0] + dx, P[1], P[2]))])


def _degenerate(b, es, c):
    """Hydrogens on the donor / on the acceptor (0/0: NaN, no bond), a collinear CB-SG-SG (NaN dihedral), a donor residue with several
    hydrogens of which one qualifies (and the same with none)."""
    handles = []
    P = b.point()
    D, A = P, (P[0] + 2.0, P[1], P[2])
    hd = b.residue("A", "GLY", [("N", "N", D), ("H", "H", D)])
    ha = b.residue("B", "GLY", [("O", "O", A)])
    handles.append((hd[0], ha[0]))
    P = b.point()
    D, A = P, (P[0] + 2.5, P[1], P[2])
    hd = b.residue("A", "GLY", [("N", "N", D), ("H", "H", A)])
    ha = b.residue("B", "GLY", [("O", "O", A)])
    handles.append((hd[0], ha[0]))
    for qualifies in (True, False):
        P = b.point()
        D, A = P, (P[0] + 2.9, P[1], P[2])
        hs = [("H1", "H", (P[0] + 0.2, P[1] + 1.0, P[2])),   # angle D-H-A below 90
              ("H2", "H", (P[0] - 1.0, P[1], P[2])),         # collinear behind the donor: too far from the acceptor
              ("H3", "H", (P[0] + 0.9, P[1] + 0.3, P[2]) if qualifies else (P[0] + 0.5, P[1] + 1.3, P[2]))]
        hd = b.residue("A", "GLY", [("N", "N", D)] + hs)
        ha = b.residue("B", "GLY", [("O", "O", A)])
        handles.append((hd[0], ha[0]))
    P = b.point()
    dss = 2.06 + (c / 2.0 if c > 0 else 0.0)
    h1 = b.residue("A", "CYS", [("CB", "C", (P[0] - 1.8, P[1], P[2])), ("SG", "S", P)])
    h2 = b.residue("B", "CYS", [("SG", "S", (P[0] + dss, P[1], P[2])), ("CB", "C", (P[0] + dss + 0.6, P[1] + 1.7, P[2]))])
    handles.append((h1[1], h2[0]))
    es.sweeps.append(Sweep("degenerate", handles, 0.0, False))


FAMILIES = ("radii", "rules")
PLACES = ("origin", "far+", "far-")


@functools.lru_cache(maxsize=None)
def gen_edges(family: str, vdw_comp: float, place: str = "origin") -> EdgeSet:
    """family "radii": clash / covalent / van der Waals bounds of every element-class pair (15 x 16 / 2, hydrogens excluded) x three
    directions x nine offsets; "rules": 3.5 / 4.0 / 4.5, the cutoffs, the H..acceptor bound, angles, dihedrals, f32 midpoints and the
    degenerate cases.  place: "origin" (lattice from 0), "far+" / "far-" (the set next to +-9999 A, an inert anchor atom at the opposite
    corner so that the box -- and with it the prefilter margin -- spans the whole +-10^4 A)."""
    es = EdgeSet(family, vdw_comp, place)
    n_slots = 120 * 3 * 3 * 9 if family == "radii" else 2000
    side = max(1, math.ceil(n_slots ** (1.0 / 3.0)))
    ext = SPACING * side
    origin = {"origin": (0.0, 0.0, 0.0), "far+": (FAR - ext, FAR - ext, FAR - ext), "far-": (-FAR, -FAR, -FAR)}[place]
    b = _Builder(origin, n_slots)
    if family == "radii":
        _radii_family(b, es, vdw_comp)
    else:
        _angle_sweeps(b, es, vdw_comp)       # first: the lattice's x = origin layer (fine ulps for the swept coordinates)
        _dihedral_sweeps(b, es, vdw_comp)
        _fixed_bounds(b, es, vdw_comp)
        _hacc_sweeps(b, es, vdw_comp)
        _f32_midpoints(b, es)
        _degenerate(b, es, vdw_comp)
    assert b.slot <= n_slots or family != "radii"
    if place != "origin":
        a = -FAR if place == "far+" else FAR
        b.residue("Z", "GLY", [("CQ", "C", (a, a, a))])
    return b.finish(es)


def vacuous(es, result, cutoff):
    """Labels of the sweeps that should show both outcomes under this cutoff but do not (a generator bug would make the parity trivial)."""
    bad = []
    for sw in es.sweeps:
        if not sw.live:
            continue
        if sw.kind == "cutoff":
            if sw.bound != cutoff:
                continue
        elif max(dist(es.atoms[x].xyz, es.atoms[y].xyz) for x, y in sw.pairs) > cutoff:
            continue
        if len({outcome(result, sw, k) for k in range(len(sw.pairs))}) < 2:
            bad.append(sw.label)
    return bad


def outcome(result, sweep, k):
    """What sweep k-th pair shows: its kind bits ("rule"), whether it is a candidate ("cutoff"), how its f32 distance rounds ("f32")."""
    p = sweep.pairs[k]
    r = result.get(p)
    if sweep.kind == "cutoff":
        return r is not None
    if sweep.kind == "f32":
        d = r[1]
        return float(np.float32(d)) > d
    return None if r is None else r[0]
