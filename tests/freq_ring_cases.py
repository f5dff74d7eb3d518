"""Built inputs for the ring rows of contact frequencies across frames (arp_contact_frequencies_ex with ARP_FREQ_RINGS: freq_rings.inl + the host
half in table_ens.cpp).  No product imports: tests/test_freq_rings_host.py checks the cases on the CPU (closed form == oracle loop, every case reaches
the edges it is named for), tests/test_freq_rings_gpu.py runs them on the device.

Topology.  K isolated motifs 32 A apart on a plane.  Every motif has a PHE ring (CG CD1 CD2 CE1 CE2 CZ, a regular hexagon of radius 1.39 A in the
xy plane) in chain A, which never moves, and a partner in chain B that the schedule places per frame:
  "rr"   a second PHE ring: centre at distance d from A's centre, the offset at angle theta against A's normal, the planes at dihedral delta
  "alt"  as "rr", but every atom of the chain-A PHE is there twice, with altloc A and with altloc B, at the same place: two ring entities, one plane
  "rc"   one LYS NZ at distance h from A's centre, the offset at angle theta against A's normal
File order: all chain-A residues (motif order), then chain B: `pads` lone LYS NZ atoms far from everything (candidates of the ring - cation sweep
that never hit: they push the motifs' NZ atoms to high candidate numbers), then the partners in motif order.  So the ring entities are: chain A's
in motif order ("alt" gives two), then chain B's rings in motif order; a row runs from the chain-A ring to the partner.

Frames.  Motif p is in state (f + 3 p) % (number of its states) in frame f:

  rr / alt   delta  theta  d (A)   result                       rc   h (A)  theta  result
             0      10     4.0     PiSandwichStacking                3.5    10     CationPi
             0      45     4.0     PiDisplacedStacking               3.5    45     none
             0      80     4.0     PiParallelInPlaneStacking         5.0    10     none
             45     (20)   4.0     PiTiltedStacking
             80     45     4.0     PiLStacking
             80     10     4.8     PiTStacking
             80     10     5.5     none
             (40)   (20)   6.5     none (centres more than 6 A apart)

Every state is at least 2 degrees and 0.05 A from every threshold of the ladder.  The thresholds themselves -- on the table path and through these
kernels, frame by frame -- are the cases of tests/ring_edge_rules.py (tests/test_ring_edge_host.py, tests/test_ring_edge_gpu.py).

expected(case) is the closed form from the schedule: one row per (motif, code) that some frame has, with the count, f32(count / F) divided in f64,
and the smallest and largest d (h) of those frames.  edges(case, per) says which edges of the two kernels a run with `per` frames per pass reaches.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import synth

SPACING, RADIUS = 32.0, 1.39
RING_NAMES = ("CG", "CD1", "CD2", "CE1", "CE2", "CZ")
CODES = {"PiDisplacedStacking": 11, "PiTStacking": 12, "PiSandwichStacking": 13, "PiParallelInPlaneStacking": 14, "PiTiltedStacking": 15,
         "PiLStacking": 16, "CationPi": 17}
RR_STATES = [(0.0, 10.0, 4.0, "PiSandwichStacking"), (0.0, 45.0, 4.0, "PiDisplacedStacking"), (0.0, 80.0, 4.0, "PiParallelInPlaneStacking"),
             (45.0, 20.0, 4.0, "PiTiltedStacking"), (80.0, 45.0, 4.0, "PiLStacking"), (80.0, 10.0, 4.8, "PiTStacking"), (80.0, 10.0, 5.5, None),
             (40.0, 20.0, 6.5, None)]
RC_STATES = [(3.5, 10.0, "CationPi"), (3.5, 45.0, None), (5.0, 10.0, None)]
RING_TILE = 64  # ring entities per workgroup of k_freq_ring_rows (freq.inl kFreqRingTile)
FIT_BLOCK, ROWS_BLOCK = 128, 256


def hexagon(centre, normal_angle_deg: float) -> np.ndarray:
    """[6, 3]: a regular hexagon around `centre` whose normal is z turned by the angle about y."""
    a = np.deg2rad(normal_angle_deg)
    u, v = np.array([np.cos(a), 0.0, -np.sin(a)]), np.array([0.0, 1.0, 0.0])
    phi = np.deg2rad(60.0 * np.arange(6))
    return np.asarray(centre)[None] + RADIUS * (np.cos(phi)[:, None] * u[None] + np.sin(phi)[:, None] * v[None])


def offset(dist: float, theta_deg: float) -> np.ndarray:
    t = np.deg2rad(theta_deg)
    return dist * np.array([np.sin(t), 0.0, np.cos(t)])


@dataclass
class Case:
    name: str
    kinds: tuple       # per motif: "rr", "alt", "rc"
    F: int
    pads: int
    rec: dict          # the topology's records (frame 0's coordinates)
    frames: np.ndarray  # [F, N, 3]
    a_atoms: list      # per motif: first atom of its chain-A residue
    b_atoms: list      # per motif: first atom of its partner
    a_ring: list       # per motif: its chain-A ring entities
    b_ring: list       # per motif: its chain-B ring entity, or -1
    n_rings: int
    n_slots: int       # ring residues

    @property
    def n(self) -> int:
        return len(self.rec["x"])

    def state(self, f: int, p: int):
        st = RC_STATES if self.kinds[p] == "rc" else RR_STATES
        return st[(f + 3 * p) % len(st)]

    def per_for_passes(self, passes: int) -> int:
        return -(-self.F // passes)


def build(name: str, kinds, F: int, pads: int = 0) -> Case:
    kinds = tuple(kinds)
    K = len(kinds)
    side = max(1, int(np.ceil(np.sqrt(K))))
    cols = {k: [] for k in ("x", "y", "z", "occupancy", "serial", "resi", "name", "resn", "chain", "altloc", "icode", "element", "model_serial")}

    def add(resn, name_, elem, chain, resi, altloc, xyz):
        k = len(cols["x"])
        for c, v in (("x", xyz[0]), ("y", xyz[1]), ("z", xyz[2]), ("occupancy", 1.0), ("serial", k + 1), ("resi", resi), ("name", name_), ("resn", resn),
                     ("chain", chain), ("altloc", altloc), ("icode", ""), ("element", elem), ("model_serial", 0)):
            cols[c].append(v)

    centres = [np.array([SPACING * (p % side), SPACING * (p // side), 0.0]) for p in range(K)]
    a_atoms, b_atoms, a_ring, b_ring = [], [-1] * K, [], [-1] * K
    n_ent = 0
    for p, kind in enumerate(kinds):  # chain A
        a_atoms.append(len(cols["x"]))
        pts = hexagon(centres[p], 0.0)
        for alt in (("A", "B") if kind == "alt" else ("",)):
            for nm, q in zip(RING_NAMES, pts):
                add("PHE", nm, "C", "A", p + 1, alt, q)
        a_ring.append([n_ent, n_ent + 1] if kind == "alt" else [n_ent])
        n_ent += 2 if kind == "alt" else 1
    pad_side = max(1, int(np.ceil(np.sqrt(max(pads, 1)))))
    for q in range(pads):  # chain B: lone LYS NZ atoms, 8 A apart (beyond any cutoff used), 64 A above the motifs
        add("LYS", "NZ", "N", "B", q + 1, "", (8.0 * (q % pad_side), 8.0 * (q // pad_side), 64.0))
    for p, kind in enumerate(kinds):  # chain B: the partners, at their places of frame 0 (frames() moves them)
        b_atoms[p] = len(cols["x"])
        if kind == "rc":
            add("LYS", "NZ", "N", "B", pads + p + 1, "", centres[p])
        else:
            for nm in RING_NAMES:
                add("PHE", nm, "C", "B", pads + p + 1, "", centres[p])
            b_ring[p] = n_ent
            n_ent += 1
    rec = synth._finish(cols)
    n_slots = K + sum(k != "rc" for k in kinds)
    case = Case(name, kinds, F, pads, rec, np.zeros((F, len(rec["x"]), 3)), a_atoms, b_atoms, a_ring, b_ring, n_ent, n_slots)
    base = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    fr = np.broadcast_to(base, (F,) + base.shape).copy()
    for f in range(F):
        for p, kind in enumerate(kinds):
            st = case.state(f, p)
            if kind == "rc":
                fr[f, b_atoms[p]] = centres[p] + offset(st[0], st[1])
            else:
                fr[f, b_atoms[p]:b_atoms[p] + 6] = hexagon(centres[p] + offset(st[2], st[1]), st[0])
    case.frames = fr
    case.rec = dict(rec, x=fr[0, :, 0].copy(), y=fr[0, :, 1].copy(), z=fr[0, :, 2].copy())
    return case


def frame_records(case: Case, f: int, frames: np.ndarray | None = None) -> dict:
    fr = case.frames if frames is None else frames
    return dict(case.rec, x=fr[f, :, 0].copy(), y=fr[f, :, 1].copy(), z=fr[f, :, 2].copy())


def expected(case: Case, ring_ring_only: bool = False) -> dict:
    """The closed-form ring rows, ordered by (from entity, to entity, code).  Columns: interaction, from_ring, to_ring, from_atom, to_atom,
    from_chain / from_resi / from_altloc, to_chain / to_resi / to_atomn, n_frames, frequency, min_distance / max_distance (f64: the schedule's)."""
    rows = []
    for p, kind in enumerate(case.kinds):
        hits = {}
        for f in range(case.F):
            st = case.state(f, p)
            code, dist = (st[2], st[0]) if kind == "rc" else (st[3], st[2])
            if code is not None:
                hits.setdefault(CODES[code], []).append(dist)
        if kind == "rc" and ring_ring_only:
            continue
        for k, e in enumerate(case.a_ring[p]):
            for code, d in hits.items():
                rows.append(dict(from_ent=case.n + e, to_ent=case.b_atoms[p] if kind == "rc" else case.n + case.b_ring[p], interaction=code, from_ring=e,
                                 to_ring=-1 if kind == "rc" else case.b_ring[p], from_atom=-1, to_atom=case.b_atoms[p] if kind == "rc" else -1,
                                 from_chain=b"A", from_resi=p + 1, from_altloc=(b"A", b"B")[k] if kind == "alt" else b"", to_chain=b"B",
                                 to_resi=case.pads + p + 1, to_atomn=b"NZ" if kind == "rc" else b"Ring", n_frames=len(d),
                                 frequency=np.float32(len(d) / case.F), min_distance=min(d), max_distance=max(d)))
    rows.sort(key=lambda r: (r["from_ent"], r["to_ent"], r["interaction"]))
    cols = ("interaction", "from_ring", "to_ring", "from_atom", "to_atom", "from_chain", "from_resi", "from_altloc", "to_chain", "to_resi", "to_atomn", "n_frames",
            "frequency", "min_distance", "max_distance")
    return {c: np.array([r[c] for r in rows]) for c in cols}


def items_per_frame(case: Case) -> np.ndarray:
    """Ring items frame by frame (an "alt" motif's hit is two items)."""
    out = np.zeros(case.F, np.int64)
    for f in range(case.F):
        for p, kind in enumerate(case.kinds):
            st = case.state(f, p)
            if (st[2] if kind == "rc" else st[3]) is not None:
                out[f] += len(case.a_ring[p])
    return out


def edges(case: Case, per: int) -> set:
    """The edges of k_freq_ring_fit / k_freq_ring_rows that a run with `per` frames per pass reaches:
      fit64 / fit128 / fit256   a pass's (frames x ring residues) threads go past one wave / one 128-thread block / 256 threads
      partial                   the last pass is shorter than the others, and there are at least three
      items64 / items256        the ring items of one pass number more than a wave / a 256-thread block of the appending kernel
      tile2                     a hit whose `from` ring is in the second or a later tile of RING_TILE entities (a second workgroup per frame)
      ring64 / ring256          a ring - ring hit whose `to` ring is swept by a lane of the second wave / in the second sweep step of the block
      cand64 / cand256          the same for the candidate number of a CationPi hit's atom
      keybit                    a hit whose `from` entity n + e needs a key bit that no atom index needs (the sorted bit range must cover n + n_rings)"""
    out = set()
    passes = [(f0, min(case.F, f0 + per)) for f0 in range(0, case.F, per)]
    fit = max((b - a) * case.n_slots for a, b in passes)
    out |= {f"fit{k}" for k in (64, 128, 256) if fit > k}
    if len(passes) >= 3 and (passes[-1][1] - passes[-1][0]) < per:
        out.add("partial")
    ipf = items_per_frame(case)
    most = max(int(ipf[a:b].sum()) for a, b in passes)
    out |= {f"items{k}" for k in (64, 256) if most > k}
    resn = case.rec["resn"]
    atom_bits = max(1, int(np.ceil(np.log2(case.n))))  # bits that hold 0 .. n - 1
    cand = np.flatnonzero(resn == b"LYS")  # every LYS atom here is a heavy atom: a candidate, in atom order
    for p, kind in enumerate(case.kinds):
        hit_states = [s for s in (RC_STATES if kind == "rc" else RR_STATES) if s[-1] is not None]
        reached = any(case.state(f, p) in hit_states for f in range(case.F))
        if not reached:
            continue
        if max(case.a_ring[p]) >= RING_TILE:
            out.add("tile2")
        if case.n + max(case.a_ring[p]) >= 1 << atom_bits:
            out.add("keybit")
        if kind == "rc":
            c = int(np.searchsorted(cand, case.b_atoms[p]))
            out |= {f"cand{k}" for k in (64, 256) if c >= k}
        else:
            out |= {f"ring{k}" for k in (64, 256) if case.b_ring[p] >= k}
    return out


@functools.lru_cache(maxsize=None)
def small_case() -> Case:
    """K = 12, F = 70: in one pass and again in three (24 + 24 + 22 frames) the fits go past 64, 128 and 256 threads; the ring items of a pass go
    past a wave in both and past 256 in one pass.  120 lone atoms bring the topology to 250 atoms: its 21 rings are entities 250 .. 270, across 256."""
    c = build("small", ["rr"] * 4 + ["rc"] * 2 + ["alt"] + ["rr"] * 3 + ["rc"] * 2, F=70, pads=120)
    assert c.n == 250 and c.n_rings == 21
    one, three = edges(c, c.F), edges(c, c.per_for_passes(3))
    assert {"fit64", "fit128", "fit256", "items64", "items256", "keybit"} <= one, one
    assert {"fit64", "fit128", "fit256", "items64", "partial", "keybit"} <= three, three
    return c


@functools.lru_cache(maxsize=None)
def wide_case() -> Case:
    """292 ring entities in five tiles and 309 candidate atoms, few frames: hits from the second tile on, `to` rings and candidate atoms swept by
    the second wave and in the second sweep step of the 256-thread block."""
    kinds = ["rr"] * 70 + ["alt"] + ["rc"] * 9 + ["rr"] * 70
    c = build("wide", kinds, F=7, pads=300)
    assert c.n_rings == 292 and c.n_rings > ROWS_BLOCK and c.n_rings > 4 * RING_TILE
    want = {"fit64", "fit128", "fit256", "items64", "items256", "tile2", "ring64", "ring256", "cand64", "cand256"}
    one, three = edges(c, c.F), edges(c, c.per_for_passes(3))
    assert want <= one, want - one
    assert want | {"partial"} <= three, (want | {"partial"}) - three
    return c


def all_cases() -> list:
    return [small_case(), wide_case()]


def min_distance_between_residues(case: Case) -> float:
    """Smallest distance between atoms of different residues over all frames (what dist_cutoff must stay below for a table without atom rows)."""
    key = np.char.add(case.rec["chain"].astype("U8"), case.rec["resi"].astype("U12"))
    _, res = np.unique(key, return_inverse=True)
    best = np.inf
    for p in range(len(case.kinds)):  # motifs are 32 A apart: only a motif's own two residues come close
        a = np.flatnonzero(res == res[case.a_atoms[p]])
        b = np.flatnonzero(res == res[case.b_atoms[p]])
        d = np.linalg.norm(case.frames[:, a][:, :, None] - case.frames[:, b][:, None], axis=-1)
        best = min(best, float(d.min()))
    return best
