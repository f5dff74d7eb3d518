"""Cases and an independent restatement for the secondary-structure call (arp_dssp: dssp.inl + the host half and the host twin in dssp.cpp).  No product imports:
tests/test_dssp_host.py checks arp_dssp_host and the input checks on the CPU, tests/test_dssp_gpu.py compares the device with arp_dssp_host.

A case is {"res": [(resn, chain, resi)], "xyz": [F, R, 4, 3] f64 (N, CA, C, O of every residue), "flags": u1 [R]}.  records(case) turns it into a topology of
the 4 R backbone atoms (frames: xyz.reshape(F, 4 R, 3)), so that the product's own backbone_select sees it as it would see a file.

margins(xyz, flags) is numpy and shares no code with the C twin.  It returns how close the case comes to each decision threshold of the definition:
  E     min |E(i, j) + 0.5| over every acceptor i and donor j that get an energy (i != j, i != j - 1, |CA - CA| < 9, j has an amide hydrogen)
  CA    min ||CA_i - CA_j| - 9| over i != j
  CN    min ||C[r-1] - N[r]| - 2.5| over the residues r that are not a chain start
  d     min |d - 0.5| over the four distances of every pair that gets an energy
  cos   min |cos kappa_k - cos 70 deg| over 2 <= k < R - 2
A device-equals-host comparison is only meaningful where none of them is within rounding of 0: every case used for one has all five >= MIN_MARGIN = 10^-6,
eight orders above the f64 rounding of these expressions (about 10^-15 relative).  A jittered case that misses it is built again with the next seed; at most
one seed in ten may be skipped that way (asserted where the cases are built).

The sweep's constants (dssp.inl): TILE = 64 donors per workgroup = acceptors per LDS tile.
"""
from __future__ import annotations

from functools import lru_cache
from pathlib import Path

import numpy as np

import trajectory_shapes as ts

DATA = Path(__file__).resolve().parent / "data"
TILE = 64
MIN_MARGIN = 1e-6
CHAIN_START, NO_H = 1, 2
SS = "-HBEGITS"
COS70 = 0.3420201433256687

# pinned (the issue's CPU restatement; the host twin reproduces them)
UBQ_STRING = "-EEEEEETTS-EEEEE--TTSBHHHHHHHHHHHH---GGGEEEEETTEE--TTSBTGGGT--TT-EEEEEE--S--"
UBQ_COUNTS = [16, 12, 2, 24, 6, 0, 12, 4]          # "-HBEGITS"
UBQ_HBONDS = 54
BFT_COUNTS = [233, 49, 24, 521, 45, 0, 112, 71]
BFT_HBONDS = 682
BFT_RESIDUES, BFT_CHAINS = 1055, 6


# ---- topology ------------------------------------------------------------------------------------------------------------------------------------------------
def flags_of(res: list) -> np.ndarray:
    f = np.zeros(len(res), "u1")
    for r, (resn, chain, _) in enumerate(res):
        if r == 0 or chain != res[r - 1][1]:
            f[r] |= CHAIN_START
        if resn == "PRO":
            f[r] |= NO_H
    return f


def case_of(res: list, xyz: np.ndarray) -> dict:
    xyz = np.asarray(xyz, np.float64)
    if xyz.ndim == 3:
        xyz = xyz[None]
    assert xyz.shape[1:] == (len(res), 4, 3)
    return {"res": list(res), "xyz": xyz, "flags": flags_of(res)}


def records(case: dict) -> dict:
    """Topology records of the case's 4 R backbone atoms at frame 0's coordinates (Structure.from_records takes them)."""
    atoms = []
    for r, (resn, chain, resi) in enumerate(case["res"]):
        for a, (name, elem) in enumerate((("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"))):
            atoms.append((resn, name, elem, chain, resi, tuple(case["xyz"][0, r, a])))
    return ts.records(atoms)


def model_records(case: dict) -> dict:
    """The same with every frame as a model of its own (a multi-model structure whose models are the frames)."""
    F, R = case["xyz"].shape[:2]
    atoms = []
    for f in range(F):
        for r, (resn, chain, resi) in enumerate(case["res"]):
            for a, (name, elem) in enumerate((("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"))):
                atoms.append((resn, name, elem, chain, resi, tuple(case["xyz"][f, r, a])))
    rec = ts.records(atoms)
    rec["serial"] = np.tile(np.arange(1, 4 * R + 1), F).astype(rec["serial"].dtype)
    rec["model_serial"] = np.repeat(np.arange(1, F + 1), 4 * R).astype(rec["model_serial"].dtype)
    return rec


def frames_of(case: dict) -> np.ndarray:
    F, R = case["xyz"].shape[:2]
    return np.ascontiguousarray(case["xyz"].reshape(F, 4 * R, 3))


# ---- the two files, parsed here ------------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _pdb(name: str):
    rows, seen = [], {}
    for line in (DATA / name).read_text().splitlines():
        if not line.startswith(("ATOM  ", "HETATM")):
            continue
        resn, chain, resi, icode, atom = line[17:20].strip(), line[21], int(line[22:26]), line[26].strip(), line[12:16].strip()
        if resn == "HOH":
            continue
        key = (chain, resi, icode)
        if not rows or rows[-1][0] != key:
            rows.append((key, resn, {}))
        rows[-1][2].setdefault(atom, (float(line[30:38]), float(line[38:46]), float(line[46:54])))
    rows = [r for r in rows if all(a in r[2] for a in ("N", "CA", "C", "O"))]
    res = [(resn, key[0], key[1]) for key, resn, _ in rows]
    xyz = np.array([[at[a] for a in ("N", "CA", "C", "O")] for _, _, at in rows], np.float64)
    xyz.setflags(write=False)
    return res, xyz


def pdb_case(name: str) -> dict:
    res, xyz = _pdb(name)
    return case_of(res, xyz)


def fragment(case: dict, keep) -> dict:
    """The residues whose (chain, resi) satisfy keep(chain, resi), in order."""
    rows = [r for r, (_, chain, resi) in enumerate(case["res"]) if keep(chain, resi)]
    return case_of([case["res"][r] for r in rows], case["xyz"][:, rows])


def first_residues(case: dict, n: int) -> dict:
    return case_of(case["res"][:n], case["xyz"][:, :n])


# ---- built backbones ---------------------------------------------------------------------------------------------------------------------------------------------
BOND_N_CA, BOND_CA_C, BOND_C_N, BOND_C_O = 1.458, 1.525, 1.329, 1.231
ANGLE_N_CA_C, ANGLE_CA_C_N, ANGLE_C_N_CA, ANGLE_CA_C_O = 111.0, 116.2, 121.7, 120.8


def place(a, b, c, bond: float, angle: float, torsion: float) -> np.ndarray:
    """NeRF: the point d with |c d| = bond, angle b-c-d and torsion a-b-c-d (degrees)."""
    ang, tor = np.radians(angle), np.radians(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    return c + bond * (-np.cos(ang) * bc + np.sin(ang) * np.cos(tor) * m + np.sin(ang) * np.sin(tor) * n)


def backbone(phi_psi: list, omega: float = 180.0) -> np.ndarray:
    """[R, 4, 3]: N, CA, C, O of a chain with the given (phi, psi) per residue, standard bond lengths and angles."""
    R = len(phi_psi)
    xyz = np.zeros((R, 4, 3))
    xyz[0, 0] = (0.0, 0.0, 0.0)
    xyz[0, 1] = (BOND_N_CA, 0.0, 0.0)
    ang = np.radians(ANGLE_N_CA_C)
    xyz[0, 2] = xyz[0, 1] + BOND_CA_C * np.array([-np.cos(ang), np.sin(ang), 0.0])
    for r in range(R):
        phi, psi = phi_psi[r]
        if r:
            xyz[r, 0] = place(xyz[r - 1, 0], xyz[r - 1, 1], xyz[r - 1, 2], BOND_C_N, ANGLE_CA_C_N, phi_psi[r - 1][1])
            xyz[r, 1] = place(xyz[r - 1, 1], xyz[r - 1, 2], xyz[r, 0], BOND_N_CA, ANGLE_C_N_CA, omega)
            xyz[r, 2] = place(xyz[r - 1, 2], xyz[r, 0], xyz[r, 1], BOND_CA_C, ANGLE_N_CA_C, phi)
        xyz[r, 3] = place(xyz[r, 0], xyz[r, 1], xyz[r, 2], BOND_C_O, ANGLE_CA_C_O, psi + 180.0)
    return xyz


HELIX_RESIDUES = 12
HELIX_ANGLES = {"alpha": (-57.0, -47.0), "310": (-49.0, -26.0), "pi": (-57.0, -70.0)}   # (phi, psi) as used; the host test records what each gives


def helix(kind: str, R: int = HELIX_RESIDUES, resn: str = "ALA") -> dict:
    return case_of([(resn, "A", k + 1) for k in range(R)], backbone([HELIX_ANGLES[kind]] * R))


# ---- the restatement: energies and margins -----------------------------------------------------------------------------------------------------------------------
def _norm(v):
    return np.sqrt((v * v).sum(-1))


def geometry(x: np.ndarray, flags: np.ndarray) -> dict:
    """One frame [R, 4, 3]: brk, donor, H, the energy matrix E[i, j] (NaN where the pair gets none), the four distance matrices."""
    R = len(x)
    N, CA, C_, O = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    cn = np.full(R, np.inf)
    cn[1:] = _norm(C_[:-1] - N[1:])
    start = (flags & CHAIN_START).astype(bool)
    start[0] = True
    brk = start | (cn > 2.5)
    donor = ~brk & ~(flags & NO_H).astype(bool)
    H = np.full((R, 3), np.nan)
    co = np.zeros((R, 3))
    co[1:] = C_[:-1] - O[:-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        H[donor] = N[donor] + co[donor] / _norm(co[donor])[:, None]
    d_ca = _norm(CA[:, None] - CA[None])
    i, j = np.indices((R, R))
    pair = (i != j) & (i != j - 1) & (d_ca < 9.0) & donor[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = {"ON": _norm(O[:, None] - N[None]), "CH": _norm(C_[:, None] - H[None]), "OH": _norm(O[:, None] - H[None]), "CN": _norm(C_[:, None] - N[None])}
        E = 27.888 * (1.0 / d["ON"] + 1.0 / d["CH"] - 1.0 / d["OH"] - 1.0 / d["CN"])
    close = np.zeros((R, R), bool)
    for v in d.values():
        close |= v < 0.5
    E = np.where(close, -9.9, E)
    E = np.where(pair, E, np.nan)
    return {"brk": brk, "donor": donor, "H": H, "E": E, "pair": pair, "d": d, "d_ca": d_ca, "cn": cn, "start": start}


def margins(xyz: np.ndarray, flags: np.ndarray) -> dict:
    xyz = np.asarray(xyz, np.float64)
    if xyz.ndim == 3:
        xyz = xyz[None]
    out = {"E": np.inf, "CA": np.inf, "CN": np.inf, "d": np.inf, "cos": np.inf}
    for x in xyz:
        g = geometry(x, np.asarray(flags))
        R = len(x)
        if g["pair"].any():
            out["E"] = min(out["E"], float(np.abs(g["E"][g["pair"]] + 0.5).min()))
            out["d"] = min(out["d"], min(float(np.abs(v[g["pair"]] - 0.5).min()) for v in g["d"].values()))
        off = ~np.eye(R, dtype=bool)
        if off.any():
            out["CA"] = min(out["CA"], float(np.abs(g["d_ca"][off] - 9.0).min()))
        inner = ~g["start"]
        if inner.any():
            out["CN"] = min(out["CN"], float(np.abs(g["cn"][inner] - 2.5).min()))
        if R >= 5:
            CA = x[:, 1]
            u, v = CA[2:-2] - CA[:-4], CA[4:] - CA[2:-2]
            cos = (u * v).sum(1) / (_norm(u) * _norm(v))
            out["cos"] = min(out["cos"], float(np.abs(cos - COS70).min()))
    return out


def clear(xyz, flags) -> bool:
    return min(margins(xyz, flags).values()) >= MIN_MARGIN


def hbonds(x: np.ndarray, flags: np.ndarray) -> set:
    """{(acceptor i, donor j)} of one frame by the restatement: i among j's two lowest energies (the lower i on ties) and E < -0.5."""
    g = geometry(x, np.asarray(flags))
    out = set()
    for j in range(len(x)):
        col = g["E"][:, j]
        idx = [i for i in np.argsort(np.where(np.isnan(col), np.inf, col), kind="stable") if not np.isnan(col[i])][:2]
        out |= {(int(i), j) for i in idx if col[i] < -0.5}
    return out


def bridges(x: np.ndarray, flags: np.ndarray, inside=None) -> dict:
    """{"par": {(i, j)}, "anti": {(i, j)}, "E": {residues}} of one frame by the restatement.  inside: a set of residues -- only bridges whose six residues
    i - 1 .. i + 1, j - 1 .. j + 1 all lie in it are considered (what a fragment cut to `inside` can see)."""
    R = len(x)
    hb, brk = hbonds(x, flags), geometry(x, np.asarray(flags))["brk"]
    ok = lambda r: 0 <= r < R and (inside is None or r in inside)
    cont3 = lambda i: ok(i - 1) and ok(i + 1) and not brk[i] and not brk[i + 1]
    out = {"par": set(), "anti": set()}
    for i in range(R):
        for j in range(R):
            if abs(i - j) < 3 or not (ok(i) and ok(j) and cont3(i) and cont3(j)):
                continue
            if ((i - 1, j) in hb and (j, i + 1) in hb) or ((j - 1, i) in hb and (i, j + 1) in hb):
                out["par"].add((i, j))
            if ((i, j) in hb and (j, i) in hb) or ((i - 1, j + 1) in hb and (j - 1, i + 1) in hb):
                out["anti"].add((i, j))
    E = {i for (i, j) in out["par"] if (i - 1, j - 1) in out["par"] or (i + 1, j + 1) in out["par"]}
    E |= {i for (i, j) in out["anti"] if (i - 1, j + 1) in out["anti"] or (i + 1, j - 1) in out["anti"]}
    out["E"] = E
    return out


# ---- moved copies ------------------------------------------------------------------------------------------------------------------------------------------------
SKIPPED_SEEDS = []   # (case, seed) of every jittered ensemble that was built again


def jittered(case: dict, F: int, seed: int, sigma: float = ts.SIGMA) -> dict:
    """F frames of the case's first frame with N(0, sigma) per atom, from the first seed >= `seed` whose frames all clear the margins."""
    R = len(case["res"])
    base = case["xyz"][0].reshape(4 * R, 3)
    for s in range(seed, seed + 10):
        xyz = ts.jitter(base, F, s, sigma).reshape(F, R, 4, 3)
        if clear(xyz, case["flags"]):
            assert s - seed <= 1, (seed, s)    # at most one seed in ten is skipped
            if s != seed:
                SKIPPED_SEEDS.append((seed, s))
            return case_of(case["res"], xyz)
    raise AssertionError(f"no seed in {seed} .. {seed + 9} clears the margins")


def tumbled(case: dict, F: int = 5, seed: int = 2) -> dict:
    R = len(case["res"])
    return case_of(case["res"], ts.tumble(case["xyz"][0].reshape(4 * R, 3), F, seed).reshape(F, R, 4, 3))


def translated(case: dict, shift: float = 1.0e4) -> dict:
    return case_of(case["res"], case["xyz"][:1] + shift * ts.DRIFT_DIRECTION)


# ---- the cases of the device-equals-host comparison ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def device_cases() -> dict:
    ubq, bft = pdb_case("1ubq.pdb"), pdb_case("6bft.pdb")
    out = {"1ubq": ubq, "6bft": bft, "1ubq_jitter33": jittered(ubq, 33, 11)}
    for kind in HELIX_ANGLES:
        out[f"helix_{kind}"] = helix(kind)
    for n in (1, 2, 3, 4, 5):
        out[f"R{n}"] = first_residues(ubq, n)
    for n in sorted({TILE - 1, TILE, TILE + 1, 63, 64, 65, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1}):
        out[f"bft_first{n}"] = first_residues(bft, n)
    for name, case in out.items():
        case["xyz"].setflags(write=False)
        assert clear(case["xyz"], case["flags"]), (name, margins(case["xyz"], case["flags"]))
    assert len(SKIPPED_SEEDS) <= 1
    return out
