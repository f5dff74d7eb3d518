"""Helpers of the residue- / chain-level SASA tests.  Nothing here comes from the path under test: the ProtOr table is
typed in from Tsai et al. 1999 as FreeSASA lists it, MaxASA from Tien et al. 2013, the sums are sequential f64 loops, the grouping is Python."""
from __future__ import annotations

import numpy as np

import arpeggia_amd as aa
from arpeggia_amd import _lib

CLASSES = {"C3H0": 1.61, "C3H1": 1.76, "C4H1": 1.88, "C4H2": 1.88, "C4H3": 1.88, "N3H0": 1.64, "N3H1": 1.64, "N3H2": 1.64, "N4H3": 1.64,
           "O1H0": 1.42, "O2H1": 1.46, "S2H0": 1.77, "S2H1": 1.77}
_ASSIGN = """
ANY: N N3H1, CA C4H1, C C3H0, O O1H0, CB C4H2, OXT O2H1
ALA: CB C4H3
ARG: CG CD C4H2, NE N3H1, CZ C3H0, NH1 NH2 N3H2
ASN: CG C3H0, OD1 O1H0, ND2 N3H2
ASP: CG C3H0, OD1 OD2 O1H0
CYS: SG S2H1
GLN: CG C4H2, CD C3H0, OE1 O1H0, NE2 N3H2
GLU: CG C4H2, CD C3H0, OE1 OE2 O1H0
GLY: CA C4H2
HIS: CG C3H0, ND1 N3H1, CD2 C3H1, NE2 N3H1, CE1 C3H1
ILE: CB C4H1, CG1 C4H2, CG2 CD1 C4H3
LEU: CG C4H1, CD1 CD2 C4H3
LYS: CG CD CE C4H2, NZ N4H3
MET: CG C4H2, SD S2H0, CE C4H3
PHE: CG C3H0, CD1 CD2 CE1 CE2 CZ C3H1
PRO: N N3H0, CG CD C4H2
SER: OG O2H1
THR: CB C4H1, OG1 O2H1, CG2 C4H3
TRP: CG CD2 CE2 C3H0, CD1 CE3 CZ2 CZ3 CH2 C3H1, NE1 N3H1
TYR: CG CZ C3H0, CD1 CD2 CE1 CE2 C3H1, OH O2H1
VAL: CB C4H1, CG1 CG2 C4H3
"""


def _parse():
    table = {}
    for line in _ASSIGN.strip().splitlines():
        resn, rest = line.split(":")
        for group in rest.split(","):
            *atoms, cls = group.split()
            for a in atoms:
                table[(resn.strip(), a)] = CLASSES[cls]
    return table


PROTOR = _parse()
AMINO_ACIDS = sorted({r for r, _ in PROTOR} - {"ANY"})
assert len(AMINO_ACIDS) == 20
# heavy atoms of the 20 residues: the backbone (with the C-terminal OXT) plus the side chain
SIDE_CHAIN = {r: sorted(a for rr, a in PROTOR if rr == r) for r in AMINO_ACIDS}
MAX_ASA = {"ALA": 129.0, "ARG": 274.0, "ASN": 195.0, "ASP": 193.0, "CYS": 167.0, "GLU": 223.0, "GLN": 225.0, "GLY": 104.0, "HIS": 224.0, "MET": 224.0,
           "ILE": 197.0, "LEU": 201.0, "LYS": 236.0, "PHE": 240.0, "PRO": 159.0, "SER": 155.0, "THR": 172.0, "TRP": 285.0, "TYR": 263.0, "VAL": 174.0}
POLAR = {"ARG", "ASN", "ASP", "GLN", "GLU", "HIS", "LYS", "SER", "THR", "TYR"}


def vdw_radius(element: str) -> float:
    return float(aa.default_params().vdw_radius[_lib.lib.arp_element_class(element.encode())])


def protor_radius(resn: str, atomn: str, element: str):
    """(radius, fell back to the element)"""
    for key in ((resn.upper(), atomn), ("ANY", atomn)):
        if key in PROTOR:
            return PROTOR[key], False
    return vdw_radius(element), True


def table_radii(s: aa.Structure, sel, radii: str):
    """f32 radii of the selected atoms from the helper's tables, and how many fell back to the element."""
    resn = [v.decode() for v in s.strings("resn")[sel]]
    atomn = [v.decode() for v in s.strings("atomn")[sel]]
    elem = [v.decode() for v in s.strings("element")[sel]]
    if radii == "vdw":
        return np.array([vdw_radius(e) for e in elem], np.float32), 0
    got = [protor_radius(r, a, e) for r, a, e in zip(resn, atomn, elem)]
    return np.array([g[0] for g in got], np.float32), sum(g[1] for g in got)


def select_1_to_4(s: aa.Structure, chains: str = "") -> np.ndarray:
    """Steps 1-4 of arp_structure_sasa_select on a single-model file without MODEL records: there steps 4 and 5 drop nothing."""
    assert len(set(s.ints("model").tolist())) == 1 and s.ints("model")[0] == 0
    return aa.sasa_select(s, chains, 0)


def seq_sum(values) -> np.float32:
    """acc = 0.0; acc += (double)v for v in order; f32(acc).  (A Python float is an IEEE double and + rounds to nearest.)"""
    acc = 0.0
    for v in np.asarray(values, np.float32).tolist():
        acc = acc + v
    return np.float32(acc)


def protor_total_of_1ubq(s: aa.Structure) -> float:
    """The chain-level total of 1ubq restated on the CPU (tests/sasa_restatement.py) with the helper's ProtOr radii, probe 1.4, 100 points."""
    import sasa_restatement as sr

    sel = select_1_to_4(s)
    r, fell_back = table_radii(s, sel, "protor")
    assert fell_back == 0 and len(sel) == 602
    R = (r + np.float32(1.4)).astype(np.float32)
    soa = s.soa("/")
    counts = sr.atom_counts(soa["x"][sel], soa["y"][sel], soa["z"][sel], R, sr.sphere_points(100))
    return float(seq_sum(sr.sasa_from_counts(R, counts, 100)))


def segment_sums(values, start, item) -> np.ndarray:
    values = np.asarray(values, np.float32)
    values = values[None] if values.ndim == 1 else values
    out = np.zeros((len(values), len(start) - 1), np.float32)
    for r, row in enumerate(values):
        for s in range(len(start) - 1):
            out[r, s] = seq_sum(row[np.asarray(item[start[s]:start[s + 1]], np.int64)])
    return out


def residue_groups(s: aa.Structure, sel):
    """[(key, [positions in sel])] per residue (chain, resi, insertion) in order of first appearance, then sorted stably by (chain, resi, insertion)."""
    chain = [v.decode() for v in s.strings("chain")[sel]]
    resi = s.ints("resi")[sel]
    ins = [v.decode() for v in s.strings("insertion")[sel]]
    resn = [v.decode() for v in s.strings("resn")[sel]]
    groups: dict = {}
    for k in range(len(sel)):
        groups.setdefault((chain[k], int(resi[k]), ins[k]), (resn[k], []))[1].append(k)
    keys = sorted(groups, key=lambda k: (k[0].encode(), k[1], k[2].encode()))
    return [((k[0], groups[k][0], k[1], k[2]), groups[k][1]) for k in keys]


def chain_groups(s: aa.Structure, sel):
    chain = [v.decode() for v in s.strings("chain")[sel]]
    groups: dict = {}
    for k in range(len(sel)):
        groups.setdefault(chain[k], []).append(k)
    return [(c, groups[c]) for c in sorted(groups, key=lambda c: c.encode())]


def columns(table) -> dict:
    """{column: list} of a polars.DataFrame or pyarrow.Table"""
    arrow = table if hasattr(table, "column") and not hasattr(table, "to_arrow") else table.to_arrow()
    return {name: arrow.column(name).to_pylist() for name in arrow.column_names}


def atom_values(ctx, s, sel, radii, n_points, xyz=None):
    """Per-atom SASA of the selected atoms from the array call, with the helper's radii."""
    soa = s.soa("/")
    x, y, z = (soa[k][sel] for k in "xyz") if xyz is None else (np.ascontiguousarray(xyz[sel, k]) for k in range(3))
    r, _ = table_radii(s, sel, radii)
    return aa.atom_sasa(ctx, x, y, z, r, None, 1.4, n_points)[0]


def expected_levels(s, sel, values):
    res, chn = residue_groups(s, sel), chain_groups(s, sel)
    return (res, np.array([seq_sum(values[g]) for _, g in res], np.float32), chn, np.array([seq_sum(values[g]) for _, g in chn], np.float32))
