"""The definition of a water bridge (include/arpeggia_amd.h, ARP_FREQ_WATERS) restated in plain numpy, from the topology's SoA
columns (Structure.soa: attr, res_ord, chain_rank, res_id), the residue names and the frames.  It returns the triples (what arp_water_bridges lists)
and, through freq_residue_common.group_by_residue, the residue rows (what ARP_FREQ_WATERS adds to the residue frequency table).  Expected values
never come from the calls under test.

  water atom   residue name HOH, not hydrogen
  polar atom   donor or acceptor, not hydrogen (never a water atom: asserted)
  leg (w, p)   dx*dx + dy*dy + dz*dz <= 12.25 in f64, in that order, inclusive
  bridge       (p, w, q), p != q, both legs, p in the ligand set, q in the receptor set, compare_residues(key(p), key(q), symmetric)
  item         (res_id[p], res_id[q], 19, frame, f32(sqrt(max(d2p, d2q))))
"""
from __future__ import annotations

import numpy as np

import arpeggia_amd as aa
from arpeggia_amd import _lib

CODE = 19
LEG2 = 12.25
TRIPLE_DTYPE = np.dtype([("frame", "<u4"), ("p", "<u4"), ("q", "<u4"), ("w", "<u4"), ("dp", "<f4"), ("dq", "<f4")])


def classify(s: aa.Structure, n: int, groups: str):
    """(soa columns cut to the topology, water [nw], polar [np]): ascending topology atom indices."""
    soa = {k: v[:n] for k, v in s.soa(groups).items() if k in ("attr", "res_ord", "chain_rank", "res_id")}
    attr = soa["attr"]
    heavy = (attr & _lib.ATTR["H"]) == 0
    water = heavy & (s.strings("resn")[:n] == b"HOH")
    polar = heavy & ((attr & (_lib.ATTR["DONOR"] | _lib.ATTR["ACCEPTOR"])) != 0)
    assert not (water & polar).any(), "a water atom with a donor or acceptor class"
    return soa, np.flatnonzero(water), np.flatnonzero(polar)


def compare_residues(soa: dict, p: int, q: int) -> bool:
    """should_compare_residues in its symmetric form (complex.rs:94-131; one model) on (chain_rank, res_ord, in ligand set, in receptor set)."""
    attr, L, R = soa["attr"], _lib.ATTR["LIGAND"], _lib.ATTR["RECEPTOR"]
    al, ar, bl, br = bool(attr[p] & L), bool(attr[p] & R), bool(attr[q] & L), bool(attr[q] & R)
    if not ((al and br) or (bl and ar)):
        return False
    ca, cb, oa, ob = int(soa["chain_rank"][p]), int(soa["chain_rank"][q]), int(soa["res_ord"][p]), int(soa["res_ord"][q])
    if ca == cb:
        return ob > 1 and oa < ob - 1
    return not (ar and br and al and bl and ca > cb)


def frame_triples(soa: dict, water: np.ndarray, polar: np.ndarray, xyz: np.ndarray, frame: int, max_partners: list | None = None) -> list:
    """The bridges of one frame, xyz [n, 3] f64, as (frame, p, q, w, d2p, d2q) tuples."""
    out = []
    if not len(water) or len(polar) < 2:
        return out
    attr, L, R = soa["attr"], _lib.ATTR["LIGAND"], _lib.ATTR["RECEPTOR"]
    P = xyz[polar]
    for w in water:
        dx, dy, dz = P[:, 0] - xyz[w, 0], P[:, 1] - xyz[w, 1], P[:, 2] - xyz[w, 2]
        d2 = dx * dx + dy * dy + dz * dz
        near = np.flatnonzero(d2 <= LEG2)
        if max_partners is not None:
            max_partners[0] = max(max_partners[0], len(near))
        for i in near:
            p = int(polar[i])
            if not attr[p] & L:
                continue
            for j in near:
                q = int(polar[j])
                if i != j and attr[q] & R and compare_residues(soa, p, q):
                    out.append((frame, p, q, int(w), float(d2[i]), float(d2[j])))
    return out


def triples(s: aa.Structure, frames: np.ndarray, groups: str, stats: dict | None = None) -> np.ndarray:
    """Every bridge of every frame, ordered by (frame, p, q, w): TRIPLE_DTYPE plus the f64 d^2 of both legs in `stats` when given."""
    frames = np.asarray(frames, np.float64)
    F, n = frames.shape[0], frames.shape[1]
    soa, water, polar = classify(s, n, groups)
    most = [0]
    rows = []
    for f in range(F):
        rows += frame_triples(soa, water, polar, frames[f], f, most)
    rows.sort(key=lambda r: r[:4])
    out = np.zeros(len(rows), TRIPLE_DTYPE)
    for k, name in enumerate(("frame", "p", "q", "w")):
        out[name] = [r[k] for r in rows]
    out["dp"] = np.sqrt(np.array([r[4] for r in rows], np.float64)).astype(np.float32)
    out["dq"] = np.sqrt(np.array([r[5] for r in rows], np.float64)).astype(np.float32)
    if stats is not None:
        stats.update(max_partners=most[0], n_water=len(water), n_polar=len(polar),
                     d2_longer=np.array([max(r[4], r[5]) for r in rows], np.float64))
    return out


def items(s: aa.Structure, frames: np.ndarray, groups: str):
    """(A, B, code, frame, f32 dist) of every bridge: what ARP_FREQ_WATERS adds to the items of the residue frequency call."""
    n = np.asarray(frames).shape[1]
    stats = {}
    t = triples(s, frames, groups, stats)
    res = s.soa("/")["res_id"][:n].astype(np.int64)
    dist = np.sqrt(stats["d2_longer"]).astype(np.float32)  # f32(sqrt(max(d2p, d2q))): the longer leg
    assert np.array_equal(dist, np.maximum(t["dp"], t["dq"]))  # (sqrt and the rounding are monotone)
    return res[t["p"].astype(np.int64)], res[t["q"].astype(np.int64)], np.full(len(t), CODE, np.int64), t["frame"].astype(np.int64), dist


def residue_rows(s: aa.Structure, frames: np.ndarray, groups: str) -> dict:
    """The code-19 rows of the residue frequency table: freq_residue_common's columns, ordered by (A, B)."""
    import freq_residue_common as fc

    frames = np.asarray(frames, np.float64)
    A, B, code, frame, dist = items(s, frames, groups)
    return fc.group_by_residue(s, frames.shape[0], frames.shape[1], A, B, code, frame, dist)


def presence(s: aa.Structure, frames: np.ndarray, groups: str) -> dict:
    """{(A, B): bool [F]}: the frames in which residue pair (A, B) is bridged."""
    frames = np.asarray(frames, np.float64)
    A, B, _, frame, _ = items(s, frames, groups)
    out = {}
    for a, b, f in zip(A.tolist(), B.tolist(), frame.tolist()):
        out.setdefault((a, b), np.zeros(frames.shape[0], bool))[f] = True
    return out


def merge(off: dict, wb: dict) -> dict:
    """The table with the flag: the flag-off table's rows and the water-bridge rows together, ordered by (from_residue, to_residue, interaction)."""
    cols = {c: np.concatenate([off[c], wb[c].astype(off[c].dtype)]) for c in off}
    order = np.lexsort((cols["interaction"], cols["to_residue"], cols["from_residue"]))
    return {c: v[order] for c, v in cols.items()}
