"""Built topologies for water bridges (ARP_FREQ_WATERS, arp_water_bridges: freq_water.inl + the host half in table_ens.cpp), each
with its expected bridges in closed form -- which (frame, p, q, w) exist and both legs, written down from the construction -- and a reach check that
the case hits the edge it is named for.  No product imports: tests/test_water_bridge_host.py checks closed form == restatement on the CPU,
tests/test_water_bridge_gpu.py runs the cases on the device.

Atoms.  A polar atom is the backbone N (donor) of a GLY residue of its own; a filler is a CA (no class); a water is the O of an HOH residue.  Residue
ordinals run in order of first appearance in the file, a chain's residue order (res_ord) in order of appearance inside the chain.  Unless a case says
otherwise, distances are multiples of 1/256 A on the axes, so d^2, its square root and the f32 of it are exact.

The kernel's constants, which the shapes straddle: 64 waters per workgroup (kFreqWaterTile), 256 polar atoms per sweep step (the workgroup),
32 partners per water (kFreqWaterPartners)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

CODE = 19
LEG = 3.5
TILE, STEP, PARTNERS = 64, 256, 32
FAR = np.array([0.0, 0.0, 900.0])
COLUMNS = ["interaction", "from_chain", "from_resn", "from_resi", "from_insertion", "to_chain", "to_resn", "to_resi", "to_insertion", "n_frames", "frequency",
           "min_distance", "max_distance", "from_residue", "to_residue"]


class Builder:
    def __init__(self):
        self.cols = {k: [] for k in ("x", "y", "z", "occupancy", "serial", "resi", "name", "resn", "chain", "altloc", "icode", "element", "model_serial")}
        self.res_of, self._res = [], {}

    def add(self, chain: str, resi: int, resn: str, name: str, elem: str, xyz) -> int:
        k = len(self.cols["x"])
        for c, v in (("x", xyz[0]), ("y", xyz[1]), ("z", xyz[2]), ("occupancy", 1.0), ("serial", k + 1), ("resi", resi), ("name", name), ("resn", resn),
                     ("chain", chain), ("altloc", ""), ("icode", ""), ("element", elem), ("model_serial", 0)):
            self.cols[c].append(v)
        self.res_of.append(self._res.setdefault((chain, resi), len(self._res)))
        return k

    def polar(self, chain, resi, xyz):
        return self.add(chain, resi, "GLY", "N", "N", xyz)

    def filler(self, chain, resi, xyz):
        return self.add(chain, resi, "GLY", "CA", "C", xyz)

    def water(self, chain, resi, xyz):
        return self.add(chain, resi, "HOH", "O", "O", xyz)

    def rec(self) -> dict:
        dt = {"x": "<f8", "y": "<f8", "z": "<f8", "occupancy": "<f8", "serial": "<i4", "resi": "<i4", "model_serial": "<i4", "name": "S8", "resn": "S8", "chain": "S8",
              "altloc": "S4", "icode": "S4", "element": "S4"}
        return {k: np.array(v, dtype=dt[k]) for k, v in self.cols.items()}


@dataclass
class Case:
    name: str
    rec: dict
    res_of: np.ndarray
    frames: np.ndarray            # [F, n, 3] f64
    groups: str
    bridges: list                 # closed form: (frame, p, q, w, d2p, d2q)
    capacity: bool = False        # the call fails with ARP_ERR_CAPACITY: no table
    timeline: dict = field(default_factory=dict)   # closed-form timeline statistics of the case's only row

    @property
    def F(self) -> int:
        return self.frames.shape[0]

    @property
    def n(self) -> int:
        return self.frames.shape[1]


def _case(name, b: Builder, groups, bridges, moves=None, F=1, **kw) -> Case:
    """moves: {frame: {atom: xyz}} on top of the builder's coordinates."""
    rec = b.rec()
    base = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    frames = np.repeat(base[None], F, axis=0)
    for f, m in (moves or {}).items():
        for a, xyz in m.items():
            frames[f, a] = xyz
    return Case(name, rec, np.array(b.res_of, np.int64), frames, groups, sorted(bridges), **kw)


def _d2(frames, f, a, w) -> float:
    d = frames[f, a] - frames[f, w]
    return float(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


# ---- closed-form tables ---------------------------------------------------------------------------------------------------------------------------
def expected_triples(c: Case) -> dict:
    """frame, p, q, w and the f32 legs, ordered by (frame, p, q, w)."""
    a = lambda k, dt: np.array([r[k] for r in c.bridges], dtype=dt)
    return {"frame": a(0, np.uint32), "p": a(1, np.uint32), "q": a(2, np.uint32), "w": a(3, np.uint32),
            "dp": np.sqrt(a(4, np.float64)).astype(np.float32), "dq": np.sqrt(a(5, np.float64)).astype(np.float32)}


def expected_rows(c: Case) -> dict:
    """The code-19 rows of the residue frequency table: per (A, B, frame) the tightest bridge's longer leg, then count, min and max over the frames."""
    per = {}
    for f, p, q, w, d2p, d2q in c.bridges:
        key = (int(c.res_of[p]), int(c.res_of[q]))
        d = np.float32(np.sqrt(max(d2p, d2q)))
        per.setdefault(key, {})
        per[key][f] = min(per[key].get(f, d), d)
    keys = sorted(per)
    first = np.array([int(np.flatnonzero(c.res_of == r)[0]) for r in range(int(c.res_of.max()) + 1)], np.int64)
    A, B = np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64)
    cnt = np.array([len(per[k]) for k in keys], np.uint32)
    out = {"interaction": np.full(len(keys), CODE, np.int32), "from_residue": A.astype(np.int32), "to_residue": B.astype(np.int32), "n_frames": cnt,
           "frequency": (cnt.astype(np.float64) / c.F).astype(np.float32),
           "min_distance": np.array([min(per[k].values()) for k in keys], np.float32), "max_distance": np.array([max(per[k].values()) for k in keys], np.float32)}
    for side, idx in (("from", first[A] if len(keys) else A), ("to", first[B] if len(keys) else B)):
        out[f"{side}_chain"] = c.rec["chain"][idx]
        out[f"{side}_resn"] = c.rec["resn"][idx]
        out[f"{side}_resi"] = c.rec["resi"][idx]
        out[f"{side}_insertion"] = c.rec["icode"][idx]
    return out


def expected_presence(c: Case) -> dict:
    out = {}
    for f, p, q, *_ in c.bridges:
        out.setdefault((int(c.res_of[p]), int(c.res_of[q])), np.zeros(c.F, bool))[f] = True
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
def legs_case() -> Case:
    """Water at the origin, partners on the axes, residues 0 and 2 of chain A.  Frame 0: both legs exactly 3.5 A -- a bridge, distance 3.5f.  Frame 1:
    q's leg at nextafter(3.5, inf) -- none.  Frame 2: q's leg at nextafter(3.5, 0) -- a bridge."""
    b = Builder()
    p = b.polar("A", 1, (LEG, 0, 0))
    b.filler("A", 2, (0, 0, 300))
    q = b.polar("A", 3, (0, LEG, 0))
    w = b.water("W", 1, (0, 0, 0))
    up, down = np.nextafter(LEG, np.inf), np.nextafter(LEG, 0.0)
    moves = {1: {q: (0, up, 0)}, 2: {q: (0, down, 0)}}
    return _case("legs", b, "/", [(0, p, q, w, LEG * LEG, LEG * LEG), (2, p, q, w, LEG * LEG, down * down)], moves, F=3)


def separation_case() -> Case:
    """Partners in residues of ord 0 (two atoms), 1, 2 and 3 of chain A around one water.  Bridges: ord 0 -> 2, 0 -> 3, 1 -> 3; never the same residue, a
    neighbour, or the reversed orientation.  The two atoms of residue 0 give two atom pairs of one residue pair: one row, n_frames 1, min_distance the
    tighter bridge's longer leg."""
    b = Builder()
    a0 = b.polar("A", 1, (3.0, 0, 0))
    a0b = b.add("A", 1, "GLY", "O", "O", (0, 3.25, 0))
    a1 = b.polar("A", 2, (-3.0, 0, 0))
    a2 = b.polar("A", 3, (0, 0, 2.75))
    a3 = b.polar("A", 4, (0, -3.375, 0))
    w = b.water("W", 1, (0, 0, 0))
    d2 = {a0: 9.0, a0b: 3.25 * 3.25, a1: 9.0, a2: 2.75 * 2.75, a3: 3.375 * 3.375}
    pairs = [(a0, a2), (a0b, a2), (a0, a3), (a0b, a3), (a1, a3)]
    return _case("separation", b, "/", [(0, p, q, w, d2[p], d2[q]) for p, q in pairs])


def chains_case(groups: str) -> Case:
    """One partner in each of chains A, B and C around a water of chain W.  "/": every chain is in both sets, each pair once, by chain order.  "A/B": A
    is the ligand -- a -> b only; C has no bit at all.  "B/A": b -> a.  "A,B/A,B": A and B in both sets -- a -> b once; C lacks the ligand bit and the
    receptor bit.  "A/A,B": b is a receptor only and a is both -- a -> b; b -> a would pass the receptor test on a and the residue rule (a is a
    ligand, b a receptor) and is refused by the ligand test on b alone."""
    b = Builder()
    pa = b.polar("A", 1, (3.0, 0, 0))
    pb = b.polar("B", 1, (0, 3.25, 0))
    pc = b.polar("C", 1, (0, 0, 2.5))
    w = b.water("W", 1, (0, 0, 0))
    d2 = {pa: 9.0, pb: 3.25 * 3.25, pc: 6.25}
    pairs = {"/": [(pa, pb), (pa, pc), (pb, pc)], "A/B": [(pa, pb)], "B/A": [(pb, pa)], "A,B/A,B": [(pa, pb)], "A/A,B": [(pa, pb)]}[groups]
    return _case(f"chains[{groups}]", b, groups, [(0, p, q, w, d2[p], d2[q]) for p, q in pairs])


def third_chain_case() -> Case:
    """The mediating water in chain C with groups "A/B", a and b 6.875 A apart: beyond dist_cutoff, and the water's legs are never listed (C is in no
    group) -- the pass has NO atom pair and still yields the row."""
    b = Builder()
    pa = b.polar("A", 1, (-3.4375, 0, 0))
    pb = b.polar("B", 1, (3.4375, 0, 0))
    w = b.water("C", 1, (0, 0, 0))
    d2 = 3.4375 * 3.4375
    return _case("third_chain_no_pair", b, "A/B", [(0, pa, pb, w, d2, d2)])


def two_waters_case() -> Case:
    """Two waters bridge the same residue pair in frame 0 (legs 3.0 and 3.25: n_frames counts the frame once, the closest approach is 3.0); in frame 1
    only the looser one does."""
    b = Builder()
    pa = b.polar("A", 1, (-3.0, 0, 0))
    pb = b.polar("B", 1, (3.0, 0, 0))
    w1 = b.water("W", 1, (0, 0, 0))
    w2 = b.water("W", 2, (0, 1.25, 0))  # 3^2 + 1.25^2 = 3.25^2
    moves = {1: {w1: FAR}}
    br = [(0, pa, pb, w1, 9.0, 9.0), (0, pa, pb, w2, 10.5625, 10.5625), (1, pa, pb, w2, 10.5625, 10.5625)]
    return _case("two_waters", b, "A/B", br, moves, F=2)


SCHEDULE_ON = [range(3, 40), range(45, 68)]


def schedule_case() -> Case:
    """70 frames (3 bitmap words): the bridge forms in frame 3, breaks in frame 40, re-forms in frame 45 and ends with frame 67."""
    b = Builder()
    pa = b.polar("A", 1, (-3.0, 0, 0))
    pb = b.polar("B", 1, (3.0, 0, 0))
    w = b.water("W", 1, (0, 0, 0))
    on = sorted(f for r in SCHEDULE_ON for f in r)
    moves = {f: {w: FAR} for f in range(70) if f not in on}
    for f in on[::2]:  # (a looser bridge in every other frame: legs of 3.25)
        moves[f] = {w: (0, 1.25, 0)}
    br = [(f, pa, pb, w, 10.5625 if f in on[::2] else 9.0, 10.5625 if f in on[::2] else 9.0) for f in on]
    return _case("schedule70", b, "A/B", br, moves, F=70, timeline={"first_frame": 3, "last_frame": 67, "n_events": 2, "longest_run": 37, "n_frames": 60})


def waters_case(n_water: int) -> Case:
    """n_water waters, 20 A apart and far from every partner but the LAST one, which bridges a and b: the tile edge at 63 / 64 / 65."""
    b = Builder()
    pa = b.polar("A", 1, (-3.0, 0, 0))
    pb = b.polar("B", 1, (3.0, 0, 0))
    for k in range(n_water - 1):
        b.water("W", k + 1, (20.0 * k, 500.0, 0))
    w = b.water("W", n_water, (0, 0, 0))
    return _case(f"waters_{n_water}", b, "A/B", [(0, pa, pb, w, 9.0, 9.0)])


def polars_case(n_polar: int) -> Case:
    """n_polar polar atoms, 10 A apart and far from the water but the last two: the sweep step at 255 / 256 / 257, the bridge's receptor at the last index."""
    b = Builder()
    for k in range(n_polar - 2):
        b.polar("A", k + 1, (10.0 * k, -500.0, 0))
    pa = b.polar("A", n_polar - 1, (-3.0, 0, 0))
    pb = b.polar("B", 1, (3.0, 0, 0))
    w = b.water("W", 1, (0, 0, 0))
    return _case(f"polars_{n_polar}", b, "A/B", [(0, pa, pb, w, 9.0, 9.0)])


def _sphere(k: int, m: int, r: float):
    z = 1.0 - 2.0 * (k + 0.5) / m
    phi = k * 2.399963229728653
    s = np.sqrt(1.0 - z * z)
    return (r * s * np.cos(phi), r * s * np.sin(phi), r * z)


def partners_case(m: int) -> Case:
    """m partners around one water, chains A and B taking turns, legs of 2.5 A + k / 64 (not on the grid: the legs are d^2 by the definition's formula).
    32: the list is full, 32 x 31 ordered candidates go through the rule and 16 x 16 bridge.  33: one too many -- ARP_ERR_CAPACITY, no table."""
    b = Builder()
    order = [k for k in range(m) if k % 2 == 0] + [k for k in range(m) if k % 2 == 1]  # (a chain's atoms follow each other in the file)
    idx = {k: b.polar("AB"[k % 2], k // 2 + 1, _sphere(k, m, 2.5 + k / 64.0)) for k in order}
    w = b.water("W", 1, (0, 0, 0))
    c = _case(f"partners_{m}", b, "A/B", [], capacity=m > PARTNERS)
    if not c.capacity:
        c.bridges = sorted((0, idx[i], idx[j], w, _d2(c.frames, 0, idx[i], w), _d2(c.frames, 0, idx[j], w)) for i in range(0, m, 2) for j in range(1, m, 2))
    return c


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = [legs_case(), separation_case()] + [chains_case(g) for g in ("/", "A/B", "B/A", "A,B/A,B", "A/A,B")] + [third_chain_case(), two_waters_case(), schedule_case()] + \
          [waters_case(k) for k in (TILE - 1, TILE, TILE + 1)] + [polars_case(k) for k in (STEP - 1, STEP, STEP + 1)] + [partners_case(PARTNERS), partners_case(PARTNERS + 1)]
    return {c.name: c for c in out}


def n_within(c: Case, f: int, w: int, polar: list) -> int:
    return sum(_d2(c.frames, f, a, w) <= LEG * LEG for a in polar)


def check_reach(name: str):
    """The precondition of a case: the construction reaches what the case is named for.  Asserted by the host test and again by the GPU test."""
    c = cases()[name]
    is_water = c.rec["resn"] == b"HOH"
    polar = [int(a) for a in np.flatnonzero((c.rec["name"] == b"N") | ((c.rec["name"] == b"O") & ~is_water))]
    waters = [int(a) for a in np.flatnonzero(is_water)]
    rows = expected_rows(c)
    if name == "legs":
        q, w = c.bridges[0][2], c.bridges[0][3]
        assert _d2(c.frames, 0, q, w) == 12.25 and _d2(c.frames, 1, q, w) > 12.25 and _d2(c.frames, 2, q, w) < 12.25
        assert np.nextafter(_d2(c.frames, 2, q, w), np.inf) <= 12.25 <= _d2(c.frames, 1, q, w)  # one step of the coordinate on either side
        assert rows["n_frames"].tolist() == [2] and rows["min_distance"].tolist() == [np.float32(3.5)] and rows["max_distance"].tolist() == [np.float32(3.5)]
    elif name == "separation":
        assert n_within(c, 0, waters[0], polar) == 5 and len(c.bridges) == 5
        assert list(zip(rows["from_residue"].tolist(), rows["to_residue"].tolist())) == [(0, 2), (0, 3), (1, 3)]
        assert rows["n_frames"].tolist() == [1, 1, 1] and rows["min_distance"][0] == np.float32(3.0)  # the tighter of 3.0 and 3.25
    elif name.startswith("chains"):
        assert n_within(c, 0, waters[0], polar) == 3
        assert len(c.bridges) == (3 if c.groups == "/" else 1)
    elif name == "third_chain_no_pair":
        pa, pb = c.bridges[0][1], c.bridges[0][2]
        assert np.linalg.norm(c.frames[0, pa] - c.frames[0, pb]) == 6.875 > 6.5 and c.rec["chain"][waters[0]] == b"C" and c.n == 3
    elif name == "two_waters":
        assert len(waters) == 2 and rows["n_frames"].tolist() == [2] and rows["min_distance"].tolist() == [np.float32(3.0)] and rows["max_distance"].tolist() == [np.float32(3.25)]
        assert sum(1 for r in c.bridges if r[0] == 0) == 2
    elif name == "schedule70":
        on = expected_presence(c)[(0, 1)]
        assert c.F == 70 and (c.F + 31) // 32 == 3 and int(on.sum()) == c.timeline["n_frames"] == 60 and on[64:68].all() and not on[68:].any()
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], on.astype(int), [0]]))))[::2]
        assert runs.tolist() == [37, 23] and c.timeline["longest_run"] == 37 and c.timeline["n_events"] == 2
        assert rows["min_distance"].tolist() == [np.float32(3.0)] and rows["max_distance"].tolist() == [np.float32(3.25)]
    elif name.startswith("waters_"):
        assert len(waters) == int(name.split("_")[1]) and c.bridges[0][3] == waters[-1] and len(c.bridges) == 1
        assert all(n_within(c, 0, w, polar) == 0 for w in waters[:-1])
    elif name.startswith("polars_"):
        assert len(polar) == int(name.split("_")[1]) and c.bridges[0][2] == polar[-1] and c.bridges[0][1] == polar[-2] and len(c.bridges) == 1
        assert n_within(c, 0, waters[0], polar) == 2
    elif name.startswith("partners_"):
        m = int(name.split("_")[1])
        assert n_within(c, 0, waters[0], polar) == m == len(polar)
        assert c.capacity == (m > PARTNERS) and (c.capacity or len(c.bridges) == (m // 2) ** 2 == 256)
    else:
        raise AssertionError(f"no reach check for {name}")
