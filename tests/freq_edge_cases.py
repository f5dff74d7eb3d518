"""Cases and references for the edges of contact frequencies across frames (arp_contact_frequencies: freq.inl + the host half in table_ens.cpp).
No product imports: tests/test_freq_edge_host.py checks the cases on the CPU (closed form == oracle loop, every case reaches the edge it is named
for), tests/test_freq_edge_gpu.py runs them on the device.

Topology.  K isolated two-atom motifs, every atom a residue of its own, the two atoms of a motif in chains A and B, motifs 32 A apart on a
plane (the second atom moves at most 8 A along x, so no pair ever forms between motifs), optionally lone atoms in front (64 A off the plane).
A motif's row runs from its chain-A atom to its chain-B atom: with A first in file order the row of motif p is (2p, 2p + 1), with B first it
is (2p + 1, 2p) (plus the lone atoms in front).

Frames.  The first atom of a motif never moves; the second sits at distance D[f, p] along x.  Every coordinate is a multiple of 1/256 A below
4096 A, so every distance and its square are exact in f32 and f64 in any evaluation order: min_distance and max_distance are compared for
exact equality.  The distance alone chooses what frame f feeds (BANDS; vdw_comp 0.1, cutoff 6.5; pinned by the oracle in the host test):

  motif                      two rows                         one row                      pair, kind == 0    no pair   coincident
  CC  ALA CB  - LEU CD1      [2.5, 3.5]    bits 3 + 18        [3.75, 4.375]   bit 18       5.5                8.0       0.0: bit 0
  ON  ASP OD1 - LYS NZ       [2.5, 3.25]   bits 3 + 4         [3.3125, 4.0]   bit 4        5.5                8.0       0.0: bit 0
  OO  SER OG  - THR OG1      [2.5, 3.0]    bits 3 + 7         [3.25, 3.5]     bit 7        5.5                8.0       0.0: bit 0

References.
  reference(top, D)       (a) closed form from the schedule: per (motif, code) the frames whose state has the code, the f32 minimum and maximum
                          of their distances, frequency = f32(count / F) divided in f64; rows ordered by (i, j, code).  No engine.
  oracle_table(top, D)    (b) one oracle atomic_contacts call per frame, aggregated in numpy.
  layout(top, D, per, cap0)  (c) what the device pipeline does with the schedule, pass by pass: listed pairs (kind != 0: the pair pass runs
                          contacts-only and drops the rest on the device), items, the runs of the sorted array
                          (thread t of k_freq_reduce is sorted position t: lane t % 64, wave t // 64, block t // 256), the two skips, and the
                          capacity of the buffers with every growth.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import synth

STEP = 1.0 / 256.0
APART, K0, ZERO = 8.0, 5.5, 0.0
CUTOFF, VDW_COMP = 6.5, 0.1
MOTIFS = {
    "CC": (("ALA", "CB", "C"), ("LEU", "CD1", "C")),
    "ON": (("ASP", "OD1", "O"), ("LYS", "NZ", "N")),
    "OO": (("SER", "OG", "O"), ("THR", "OG1", "O")),
}
# kind -> {"both": (lo, hi, codes), "one": (lo, hi, codes)}
BANDS = {
    "CC": {"both": (2.5, 3.5, (3, 18)), "one": (3.75, 4.375, (18,))},
    "ON": {"both": (2.5, 3.25, (3, 4)), "one": (3.3125, 4.0, (4,))},
    "OO": {"both": (2.5, 3.0, (3, 7)), "one": (3.25, 3.5, (7,))},
}
SPACING = 32.0
AUTO_ATOMS = 1 << 21  # atoms per pass when the knob freq_chunk_atoms is 0
MAX_FRAMES_PER_PASS = 65535
CAP_FLOOR = 1 << 16


@dataclass
class Topology:
    kinds: tuple
    order: str  # "AB": chain A first in file order; "BA": chain B first
    pads: int
    rec: dict

    @property
    def K(self) -> int:
        return len(self.kinds)

    @property
    def n(self) -> int:
        return self.pads + 2 * len(self.kinds)

    def fixed(self, p: int) -> int:
        return self.pads + 2 * p

    def moving(self, p: int) -> int:
        return self.pads + 2 * p + 1

    def row(self, p: int) -> tuple:
        """(from atom, to atom) of motif p: the chain-A atom first."""
        return (self.fixed(p), self.moving(p)) if self.order == "AB" else (self.moving(p), self.fixed(p))


def topology(kinds, order: str = "AB", pads: int = 0) -> Topology:
    assert order in ("AB", "BA")
    cols = {k: [] for k in ("x", "y", "z", "occupancy", "serial", "resi", "name", "resn", "chain", "altloc", "icode", "element", "model_serial")}

    def add(resn, name, elem, chain, x, y, z):
        k = len(cols["x"])
        for c, v in (("x", x), ("y", y), ("z", z), ("occupancy", 1.0), ("serial", k + 1), ("resi", k + 1), ("name", name), ("resn", resn),
                     ("chain", chain), ("altloc", ""), ("icode", ""), ("element", elem), ("model_serial", 0)):
            cols[c].append(v)

    K = len(kinds)
    side = max(1, int(np.ceil(np.sqrt(max(K, pads)))))
    for q in range(pads):  # lone atoms: a plane of their own, 64 A from the motifs
        add("GLY", "CA", "C", "A", SPACING * (q % side), SPACING * (q // side), 64.0)
    first, second = ("A", "B") if order == "AB" else ("B", "A")
    for p, kind in enumerate(kinds):
        a, b = MOTIFS[kind]
        x, y = SPACING * (p % side), SPACING * (p // side)
        add(*a, first, x, y, 0.0)
        add(*b, second, x, y, 0.0)
    return Topology(tuple(kinds), order, pads, synth._finish(cols))


def frames(top: Topology, D: np.ndarray) -> np.ndarray:
    """[F, n, 3] f64 coordinates of the schedule D [F, K]."""
    D = np.asarray(D, np.float64)
    assert D.ndim == 2 and D.shape[1] == top.K
    assert np.array_equal(D * 256.0, np.round(D * 256.0)) and (D >= 0).all() and (D <= APART).all()
    base = np.stack([top.rec["x"], top.rec["y"], top.rec["z"]], 1)
    out = np.broadcast_to(base, (D.shape[0],) + base.shape).copy()
    out[:, top.pads + 1::2, 0] += D
    assert (np.abs(out) < 4096.0).all()
    return out


def code_masks(top: Topology, D: np.ndarray) -> list:
    """[(i, j, code, mask [F])] for every row a motif of the topology can have, ordered by (i, j, code); every distance must be a listed state."""
    D = np.asarray(D, np.float64)
    rows = []
    for p, kind in enumerate(top.kinds):
        d = D[:, p]
        per_code = {0: d == ZERO}
        known = (d == ZERO) | (d == K0) | (d == APART)
        for lo, hi, codes in BANDS[kind].values():
            inside = (d >= lo) & (d <= hi)
            known |= inside
            for c in codes:
                per_code[c] = per_code.get(c, np.zeros(len(d), bool)) | inside
        if not known.all():
            raise ValueError(f"motif {p} ({kind}): distance {d[~known][0]} is not a state of the table")
        i, j = top.row(p)
        rows += [(i, j, c, per_code[c]) for c in sorted(per_code)]
    rows.sort(key=lambda r: r[:3])
    return rows


def has_candidate(D: np.ndarray) -> np.ndarray:
    """(frame, motif) whose atoms are within the cutoff: a candidate pair, kind == 0 included."""
    return np.asarray(D) <= CUTOFF


def listed(top: Topology, D: np.ndarray) -> np.ndarray:
    """(frame, motif) whose pair the contacts-only pair pass hands to k_freq_expand: the candidates with kind != 0.  (The pass drops a
    candidate no rule matched on the device, so a frame at 5.5 A gives the frequency kernels no pair at all.)"""
    out = np.zeros(np.asarray(D).shape, bool)
    for i, j, _, mask in code_masks(top, D):
        out[:, (min(i, j) - top.pads) // 2] |= mask
    return out


def _identity(top: Topology, i: np.ndarray, j: np.ndarray, out: dict) -> dict:
    rec = top.rec
    for side, idx in (("from", i), ("to", j)):
        out[f"{side}_chain"] = rec["chain"][idx]
        out[f"{side}_resn"] = rec["resn"][idx]
        out[f"{side}_resi"] = rec["resi"][idx]
        out[f"{side}_insertion"] = rec["icode"][idx]
        out[f"{side}_altloc"] = rec["altloc"][idx]
        out[f"{side}_atomn"] = rec["name"][idx]
        out[f"{side}_atomi"] = rec["serial"][idx]
    return out


def _table(top: Topology, F: int, rows: list) -> dict:
    """rows: [(i, j, code, count, f32 min, f32 max)] in (i, j, code) order -> the columns of the frequency table."""
    a = lambda k, dt: np.array([r[k] for r in rows], dtype=dt)
    i, j = a(0, np.int64), a(1, np.int64)
    cnt = a(3, np.uint32)
    out = {"interaction": a(2, np.int32), "from_atom": i.astype(np.int32), "to_atom": j.astype(np.int32), "n_frames": cnt,
           "frequency": (cnt.astype(np.float64) / float(F)).astype(np.float32), "min_distance": a(4, np.float32), "max_distance": a(5, np.float32)}
    return _identity(top, i, j, out)


def reference(top: Topology, D: np.ndarray) -> dict:
    """(a) the frequency table in closed form from the schedule."""
    D = np.asarray(D, np.float64)
    rows = []
    for i, j, c, mask in code_masks(top, D):
        if mask.any():
            p = (min(i, j) - top.pads) // 2
            d = D[mask, p].astype(np.float32)
            rows.append((i, j, c, int(mask.sum()), d.min(), d.max()))
    return _table(top, D.shape[0], rows)


def oracle_table(top: Topology, D: np.ndarray) -> dict:
    """(b) one oracle atomic_contacts call per frame of the schedule, aggregated by (i, j, code)."""
    import oracle_binding as ob

    xyz = frames(top, D)
    atoms = synth.records_to_oracle(top.rec, flat=False)
    agg = {}
    for f in range(xyz.shape[0]):
        atoms["x"], atoms["y"], atoms["z"] = xyz[f, :, 0], xyz[f, :, 1], xyz[f, :, 2]
        for q in ob.Structure.from_atoms(atoms, False).atomic_contacts("/", VDW_COMP, CUTOFF):
            d = np.float32(q["dist"])
            kind = int(q["kind"])
            for c in range(len(ob.INTERACTIONS)):
                if kind >> c & 1:
                    key = (int(q["i"]), int(q["j"]), c)
                    n, mn, mx = agg.get(key, (0, d, d))
                    agg[key] = (n + 1, min(mn, d), max(mx, d))
    return _table(top, xyz.shape[0], [k + agg[k] for k in sorted(agg)])


def oracle_pairs(top: Topology, D: np.ndarray) -> tuple:
    """(candidates, candidates with kind != 0) of the oracle over all frames of the schedule."""
    import oracle_binding as ob

    xyz = frames(top, D)
    atoms = synth.records_to_oracle(top.rec, flat=False)
    total = nonzero = 0
    for f in range(xyz.shape[0]):
        atoms["x"], atoms["y"], atoms["z"] = xyz[f, :, 0], xyz[f, :, 1], xyz[f, :, 2]
        p = ob.Structure.from_atoms(atoms, False).atomic_contacts("/", VDW_COMP, CUTOFF)
        total += len(p)
        nonzero += int((p["kind"] != 0).sum())
    return total, nonzero


COLUMNS = ["interaction", "from_chain", "from_resn", "from_resi", "from_insertion", "from_altloc", "from_atomn", "from_atomi", "to_chain", "to_resn",
           "to_resi", "to_insertion", "to_altloc", "to_atomn", "to_atomi", "n_frames", "frequency", "min_distance", "max_distance", "from_atom", "to_atom"]


def assert_same_table(got: dict, want: dict):
    """Every column, row order included, for exact equality (strings compared at the reference's width)."""
    assert set(got) == set(COLUMNS) and set(want) == set(COLUMNS)
    for c in COLUMNS:
        assert len(got[c]) == len(want[c]), (c, len(got[c]), len(want[c]))
        g = got[c].astype(want[c].dtype) if want[c].dtype.kind == "S" else got[c]
        if want[c].dtype.kind == "f":
            assert g.dtype == np.float32, c
            assert np.array_equal(g.view(np.uint32), want[c].astype(np.float32).view(np.uint32)), (c, g, want[c])
        else:
            assert np.array_equal(g, want[c].astype(g.dtype)), (c, g, want[c])


# ---- (c) the layout the device pipeline must produce -----------------------------------------------------------------------------------------
def frames_per_pass(n: int, F: int, chunk_atoms: int = 0) -> int:
    """device_frequencies' pass size for a topology of n atoms (every atom its own residue, no hydrogens)."""
    budget = chunk_atoms if chunk_atoms else AUTO_ATOMS
    return min(max(1, budget // n), F, 0x7FFFFFF0 // (n + 1), MAX_FRAMES_PER_PASS)


@dataclass
class Run:
    key: tuple  # (i, j, code)
    start: int
    length: int
    in_agg: bool  # one item of the run is the aggregate's

    @property
    def end(self) -> int:  # last position
        return self.start + self.length - 1


@dataclass
class Pass:
    f0: int
    frames: int
    n_pairs: int
    n_items: int
    n_agg: int          # aggregate rows before the pass
    skipped: str | None  # "no_pairs", "no_items" (unreachable from the pair pass: every listed pair has a code) or None
    allocated: bool      # the buffers were first allocated in this pass
    cap: int             # capacity when the pass expands its items (0: no buffers yet)
    grew: bool           # n_agg + n_items exceeded cap: grown with keep = n_agg, expanded again
    cap_after: int
    runs: list = field(default_factory=list)

    @property
    def m(self) -> int:
        return self.n_agg + self.n_items


def layout(top: Topology, D: np.ndarray, per: int, cap0: int = 0) -> list:
    """Pass by pass what device_frequencies does with the schedule in passes of `per` frames; cap0: the knob freq_cap_items (0: automatic)."""
    D = np.asarray(D, np.float64)
    F = D.shape[0]
    rows = code_masks(top, D)
    masks = np.stack([r[3] for r in rows]) if rows else np.zeros((0, F), bool)
    pairs = listed(top, D)
    in_agg = np.zeros(len(rows), bool)
    cap, out = 0, []
    for f0 in range(0, F, per):
        fc = min(per, F - f0)
        counts = masks[:, f0:f0 + fc].sum(1)
        n_pairs, n_items, n_agg = int(pairs[f0:f0 + fc].sum()), int(counts.sum()), int(in_agg.sum())
        ps = Pass(f0, fc, n_pairs, n_items, n_agg, None, False, cap, False, cap)
        out.append(ps)
        if n_pairs == 0:
            ps.skipped = "no_pairs"
            continue
        if cap == 0:
            cap = cap0 if cap0 > 0 else max(CAP_FLOOR, 2 * n_pairs)
            ps.allocated, ps.cap = True, cap
        if n_agg + n_items > cap:
            want = n_agg + n_items
            cap = want + want // 4
            ps.grew = True
        ps.cap_after = cap
        if n_items == 0:
            ps.skipped = "no_items"
            continue
        at = 0
        for k in np.flatnonzero(in_agg | (counts > 0)):
            length = int(in_agg[k]) + int(counts[k])
            ps.runs.append(Run(rows[k][:3], at, length, bool(in_agg[k])))
            at += length
        assert at == ps.m
        in_agg |= counts > 0
    return out


def run_edges(ps: Pass) -> set:
    """The edges of k_freq_reduce's run folding that the pass's runs reach (see RUN_EDGES)."""
    got = set()
    m = ps.m
    for r in ps.runs:
        lane = r.start % 64
        if r.length == 64 and lane == 0:
            got.add("run64_at_lane0")
        if r.length == 65 and lane == 0:
            got.add("run65_at_lane0")
        if r.length == 64 and lane == 1:
            got.add("run64_at_lane1")
        if lane == 63 and r.length > 1:
            got.add("run_from_lane63_into_next_wave")
        if r.length == 1 and lane == 63:
            got.add("single_at_lane63")
        if r.length == 1 and lane == 0:
            got.add("single_at_lane0")
        if r.start <= 255 and r.end >= 256:
            got.add("run_across_255_256")
        first_whole = -(-r.start // 64)
        if (r.end + 1) // 64 - first_whole >= 3:
            got.add("run_over_three_waves")
    if ps.runs and ps.runs[-1].end == m - 1 and m % 64 != 0 and m % 256 != 0:
        got.add("ragged_tail")
    if m and m % 256 == 0:
        got.add("m_multiple_of_256")
    if m == 1:
        got.add("m_is_1")
    return got


RUN_EDGES = {"run64_at_lane0", "run65_at_lane0", "run64_at_lane1", "run_from_lane63_into_next_wave", "single_at_lane63", "single_at_lane0",
             "run_across_255_256", "run_over_three_waves", "ragged_tail"}


# ---- schedules -------------------------------------------------------------------------------------------------------------------------------
def apart(F: int, K: int) -> np.ndarray:
    return np.full((F, K), APART)


def band_distances(kind: str, state: str, which: np.ndarray) -> np.ndarray:
    """Distances of a band, one per entry of `which` (any integers): the band's 1/256 A steps, walked with stride 37."""
    lo, hi, _ = BANDS[kind][state]
    steps = int(round((hi - lo) * 256.0)) + 1
    return lo + ((np.asarray(which, np.int64) * 37) % steps) * STEP


def put(top: Topology, D: np.ndarray, p: int, fr, state: str):
    """Motif p in the frames fr: "both", "one" (distances varied over the band by frame), "k0", "zero" or "apart"."""
    fr = np.asarray(fr, np.int64)
    if state in ("both", "one"):
        D[fr, p] = band_distances(top.kinds[p], state, fr + 11 * p)
    else:
        D[fr, p] = {"k0": K0, "zero": ZERO, "apart": APART}[state]


@dataclass
class Case:
    name: str
    top: Topology
    D: np.ndarray
    per: int | None = None   # frames per pass (freq_chunk_atoms = per * n); None: the knob stays 0
    cap: int = 0             # freq_cap_items
    oracle_frames: np.ndarray | None = None  # (b) on these frames only (None: every frame)

    @property
    def F(self) -> int:
        return self.D.shape[0]

    @property
    def chunk_atoms(self) -> int:
        return 0 if self.per is None else self.per * self.top.n

    @property
    def per_frames(self) -> int:
        return frames_per_pass(self.top.n, self.F, self.chunk_atoms)

    def layout(self, cap0: int | None = None) -> list:
        return layout(self.top, self.D, self.per_frames, self.cap if cap0 is None else cap0)


# run lengths of the lane / wave / block layout: (kind, frames with two rows, frames with one row) per motif.  Runs in key order:
#   [0,64) [64,129) | [129,191) | [191] [192] | [193,393) | [393,449) | [449,513) | [513,575) | [575,585) | [585,835)      m = 835
RUN_SPECS = [("CC", 64, 1), ("OO", 0, 62), ("ON", 1, 0), ("CC", 0, 200), ("ON", 0, 56), ("OO", 0, 64), ("CC", 0, 62), ("ON", 0, 10), ("CC", 0, 250)]
RUN_SPECS_256 = [("CC", 100, 56), ("ON", 0, 256)]  # runs 100, 156, 256: m = 512
RUN_SPECS_1 = [("OO", 0, 1)]
RUN_F = 260


def _spread(F: int, start: int, count: int) -> np.ndarray:
    return (start + np.arange(count)) % F


def run_case(name: str, specs: list, order: str, second_pass: bool, F: int = RUN_F) -> Case:
    """One pass of F frames whose sorted items form the runs of `specs`.  second_pass: F more frames in front in which every other motif
    (0, 2, 3, 5, ...: those with p % 3 != 1) is on in one frame, so that in pass 1 its runs carry the aggregate's item and have one frame less of
    their own; the motifs with p % 3 == 1 are new keys in pass 1.  The layout of pass 1 is that of the one-pass case."""
    top = topology([s[0] for s in specs], order)
    D = apart((2 if second_pass else 1) * F, top.K)
    off = F if second_pass else 0
    for p, (_, both, one) in enumerate(specs):
        carried = second_pass and p % 3 != 1
        if carried:  # the aggregate's item: the state that feeds all of the motif's rows, at the band's low or high end
            state = "both" if both else "one"
            lo, hi, _ = BANDS[top.kinds[p]][state]
            D[(5 * p) % F, p] = lo if p % 2 else hi
            both, one = (both - 1, one) if both else (both, one - 1)
        start = 17 * p
        put(top, D, p, off + _spread(F, start, both), "both")
        put(top, D, p, off + _spread(F, start + both, one), "one")
    return Case(name, top, D, per=F)


def across_case() -> Case:
    """5 passes of 16 frames, the last of 5: the keys of the 'across passes' list."""
    per, F = 16, 69
    top = topology(["CC", "ON", "OO", "CC", "ON", "OO", "CC", "ON", "CC"], "AB")
    D = apart(F, top.K)
    put(top, D, 0, [0], "one")                                   # only in frame 0
    put(top, D, 1, [F - 1], "both")                              # only in frame F - 1 (the partial pass)
    put(top, D, 2, list(range(3, 9)) + list(range(35, 44)), "one")  # passes 0 and 2, not 1
    put(top, D, 3, [65, 67], "both")                             # first appears in the last pass
    put(top, D, 4, range(F), "one")                              # every frame: frequency 1.0
    put(top, D, 5, range(2, F, 3), "one")
    D[D[:, 5] != APART, 5] = 3.375
    D[5, 5], D[66, 5] = 3.25, 3.5                                # minimum in the first pass, maximum in the last
    put(top, D, 6, range(1, F, 4), "one")
    D[D[:, 6] != APART, 6] = 4.0
    D[9, 6], D[65, 6] = 4.375, 3.75                              # maximum in the first pass, minimum in the last
    D[[3, 20, 40], 7] = 3.5                                      # minimum == maximum across frames of three passes
    put(top, D, 8, range(10, 50), "one")                         # bit 18 in 40 frames ...
    put(top, D, 8, [12, 18, 25, 31, 33, 47, 48], "both")         # ... bit 3 in 7 of them
    return Case("across_keys", top, D, per=per)


def skip_case(name: str, kinds_of_pass: str) -> Case:
    """Passes of 16 frames (the last of 5) of the kinds in kinds_of_pass: 'n' normal, 'a' every motif apart (no candidate pair), 'k' every
    motif at 5.5 A (candidates, all with kind == 0: none listed)."""
    per = 16
    F = per * (len(kinds_of_pass) - 1) + 5
    top = topology(["CC", "ON", "OO", "CC"], "BA")
    D = apart(F, top.K)
    for k, what in enumerate(kinds_of_pass):
        fr = np.arange(k * per, min((k + 1) * per, F))
        if what == "k":
            D[fr] = K0
        elif what == "n":
            for p in range(top.K):
                put(top, D, p, fr[(fr + p) % 3 == 0], "both")
                put(top, D, p, fr[(fr + p) % 3 == 1], "one")
                put(top, D, p, fr[(fr + p) % 7 == 2], "k0")
    return Case(name, top, D, per=per)


def expand_case() -> Case:
    """One pass whose pair list mixes pairs with 1 and 2 set bits and pairs with bit 0 alone (coincident atoms), among candidates with
    kind == 0 (dropped by the contacts-only pair pass: k_freq_expand sees a 0-bit lane only past n_pairs, in the tail wave) and frames without
    the pair."""
    top = topology(["CC", "ON", "OO"] * 3, "AB")
    F = 61
    D = apart(F, top.K)
    states = ["both", "one", "k0", "apart", "one", "both", "k0"]
    for f in range(F):
        for p in range(top.K):
            put(top, D, p, [f], states[(3 * f + 5 * p + f * p) % len(states)])
    D[7, :] = ZERO  # a frame of coincident atoms
    D[29, 4] = ZERO
    return Case("expand_mixed", top, D, per=F)


def capacity_case(exact: bool) -> Case:
    """Passes of 8 frames (the last of 3).  Motif 0 is on in pass 0 only and motif 1 in pass 1 only: their rows exist only in the aggregate
    when later passes grow the buffers.  exact: pass 0 has as many items as freq_cap_items holds and pass 1 needs one item more."""
    per, F = 8, 35
    top = topology(["CC", "ON", "OO", "CC", "ON", "OO"], "AB")
    D = apart(F, top.K)
    put(top, D, 0, [1, 4], "both")
    put(top, D, 0, [2], "one")
    put(top, D, 1, [9, 13], "both")
    if exact:
        # pass 0: 5 items of motif 0 + 3 of motif 2 = 8 items, 3 rows; pass 1: 3 + n_items must be 9
        put(top, D, 2, [0, 3, 6], "one")
        put(top, D, 2, [8, 15], "one")  # pass 1: 4 (motif 1) + 2 = 6 items
        for p in (3, 4, 5):
            put(top, D, p, range(16, F, 2), "both")
        return Case("capacity_exact", top, D, per=per, cap=8)
    for p in (2, 3):
        put(top, D, p, range(8, 16), "both")
    for p in (2, 3, 4, 5):
        put(top, D, p, range(16, 24), "both")
        put(top, D, p, range(24, F), "one")
    return Case("capacity_1", top, D, per=per, cap=1)


def floor_case() -> Case:
    """The natural first allocation (65 536 items, no knob for it): pass 0 has 40 items, pass 1 has 300 motifs x 128 frames x 2 rows."""
    per, F = 128, 266
    top = topology(["CC", "ON", "OO"] * 100, "AB")
    D = apart(F, top.K)
    put(top, D, 0, range(40), "one")
    for p in range(top.K):
        put(top, D, p, range(per, 2 * per), "both")
    put(top, D, 5, range(258, F), "one")
    return Case("capacity_floor", top, D, per=per)


def key_bits_case(n: int) -> Case:
    """n atoms, B first: the row of the last motif runs from atom n - 1 (for n = 2^k + 1 the index needs bit k) and must come last."""
    K = n // 2
    top = topology((["CC", "ON", "OO"] * K)[:K], "BA", pads=n - 2 * K)
    F = 5
    D = apart(F, top.K)
    for p in range(K):
        put(top, D, p, [(p + 1) % F, (p + 3) % F], "both" if p % 2 else "one")
    put(top, D, K - 1, [0, 4], "both")
    return Case(f"key_bits_{n}", top, D, per=3)


def many_frames_case() -> Case:
    """70 000 frames of four atoms: the cap of 65 535 frames per pass gives two passes (the documented contract F <= 2^40 / n at a size no other
    test has).  Motif 0 is on when f % 3 == 0, motif 1 only in frames 65 534, 65 535 and 69 999."""
    F = 70000
    top = topology(["CC", "ON"], "AB")
    D = apart(F, top.K)
    put(top, D, 0, range(0, F, 3), "both")
    put(top, D, 1, [65534, 65535, 69999], "one")
    sub = sorted({0, F - 1, MAX_FRAMES_PER_PASS - 1, MAX_FRAMES_PER_PASS} | set(range(0, F, 997)))
    return Case("many_frames", top, D, per=None, oracle_frames=np.array(sub))


def rounding_case(F: int) -> Case:
    """Rows with counts 1, F - 1 and F: frequency = f32(count / F), the quotient taken in f64."""
    top = topology(["CC", "ON", "OO"], "AB")
    D = apart(F, top.K)
    put(top, D, 0, [F // 2], "one")
    put(top, D, 1, range(1, F), "one")
    put(top, D, 2, range(F), "one")
    return Case(f"rounding_{F}", top, D, per=None if F < 100 else 300)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = []
    for order in ("AB", "BA"):
        out.append(run_case(f"runs_{order}", RUN_SPECS, order, False))
        out.append(run_case(f"runs_second_pass_{order}", RUN_SPECS, order, True))
    out += [run_case("runs_m512", RUN_SPECS_256, "AB", False), run_case("runs_m512_second_pass", RUN_SPECS_256, "BA", True),
            run_case("runs_m1", RUN_SPECS_1, "AB", False, F=3)]  # (m == 1 has no second-pass form: an aggregate row and an item make m >= 2)
    out.append(across_case())
    out += [skip_case("skip_middle", "nankn"), skip_case("skip_first_apart_k0", "aknn"), skip_case("skip_first_k0_apart", "kann"), skip_case("skip_all", "akak")]
    out.append(expand_case())
    out += [capacity_case(False), capacity_case(True), floor_case()]
    out += [key_bits_case(n) for n in (64, 65, 128, 129)]
    out.append(many_frames_case())
    out += [rounding_case(F) for F in (1, 3, 7, 2000)]
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def reference_of(name: str) -> dict:
    c = cases()[name]
    return reference(c.top, c.D)


def check_reach(name: str):
    """The precondition of a case: its layout reaches the edge it is named for.  Asserted by the host test, and again by the GPU test before
    it calls the device."""
    c = cases()[name]
    lay = c.layout()
    ref = reference_of(name)
    assert all(ps.frames <= 300 for ps in lay) or name == "many_frames"
    assert c.per_frames * c.top.n < 300000
    if name.startswith("runs_"):
        second = "second_pass" in name
        assert len(lay) == (2 if second else 1)
        ps = lay[-1]
        assert not ps.grew and ps.skipped is None
        assert (ps.n_agg > 0) == second
        if second:
            assert lay[0].skipped is None and lay[0].n_agg == 0
            one_pass = cases()[name.replace("_second_pass", "")].layout()[-1]
            assert [(r.start, r.length) for r in ps.runs] == [(r.start, r.length) for r in one_pass.runs]
            assert any(r.in_agg for r in ps.runs) and any(not r.in_agg for r in ps.runs)  # keys of the aggregate and keys new in this pass
            if ps.m == 835:
                assert any(r.in_agg and r.length == 1 for r in ps.runs)  # a key of the aggregate without items in this pass
        edges = run_edges(ps)
        if "m512" in name:
            assert ps.m == 512 and "m_multiple_of_256" in edges
        elif "m1" in name:
            assert ps.m == 1 and "m_is_1" in edges
        else:
            assert ps.m == 835 and RUN_EDGES <= edges, RUN_EDGES - edges
            assert [(r.start, r.length) for r in ps.runs] == [(0, 64), (64, 65), (129, 62), (191, 1), (192, 1), (193, 200), (393, 56), (449, 64), (513, 62),
                                                              (575, 10), (585, 250)]
    elif name == "across_keys":
        F, per = c.F, c.per
        assert len(lay) == 5 and lay[-1].frames == 5 and all(ps.skipped is None for ps in lay)
        masks = {r[:3]: r[3] for r in code_masks(c.top, c.D)}
        passes_of = lambda key: sorted(set((np.flatnonzero(masks[key]) // per).tolist()))
        row = c.top.row
        assert np.flatnonzero(masks[row(0) + (18,)]).tolist() == [0]
        assert np.flatnonzero(masks[row(1) + (4,)]).tolist() == [F - 1] and np.flatnonzero(masks[row(1) + (3,)]).tolist() == [F - 1]
        assert passes_of(row(2) + (7,)) == [0, 2]
        assert passes_of(row(3) + (18,)) == [4]
        assert masks[row(4) + (4,)].all()
        d5, d6 = c.D[:, 5], c.D[:, 6]
        on5, on6 = d5 != APART, d6 != APART
        assert np.flatnonzero(d5 == d5[on5].min()).tolist() == [5] and np.flatnonzero(d5 == d5[on5].max()).tolist() == [66]
        assert np.flatnonzero(d6 == d6[on6].max()).tolist() == [9] and np.flatnonzero(d6 == d6[on6].min()).tolist() == [65]
        assert masks[row(7) + (4,)].sum() == 3 and len(passes_of(row(7) + (4,))) == 3
        assert masks[row(8) + (18,)].sum() == 40 and masks[row(8) + (3,)].sum() == 7
        k = {(int(i), int(j), int(cd)): r for r, (i, j, cd) in enumerate(zip(ref["from_atom"], ref["to_atom"], ref["interaction"]))}
        assert ref["frequency"][k[row(4) + (4,)]] == np.float32(1.0)
        r7 = k[row(7) + (4,)]
        assert ref["min_distance"][r7] == ref["max_distance"][r7] and ref["n_frames"][r7] == 3
    elif name.startswith("skip_"):
        kinds = {"skip_middle": "nankn", "skip_first_apart_k0": "aknn", "skip_first_k0_apart": "kann", "skip_all": "akak"}[name]
        # a pass at 5.5 A has candidates but no listed pair (contacts-only): both kinds of pass leave through `if (n_pairs == 0) continue`
        want = {"n": None, "a": "no_pairs", "k": "no_pairs"}
        assert [ps.skipped for ps in lay] == [want[k] for k in kinds] and lay[-1].frames == 5
        cand = has_candidate(c.D)
        for k, ps in zip(kinds, lay):
            assert (k == "k") == (ps.n_pairs == 0 and cand[ps.f0:ps.f0 + ps.frames].all()) and (k == "a") == (not cand[ps.f0:ps.f0 + ps.frames].any())
        # the buffers are allocated by the first pass that has listed pairs
        if name == "skip_all":
            assert len(ref["n_frames"]) == 0 and not any(ps.allocated for ps in lay)
        else:
            assert [ps.allocated for ps in lay].index(True) == kinds.index("n")
        if name.startswith("skip_first"):  # the buffers are first allocated in pass 2
            assert lay[2].allocated and lay[2].n_agg == 0 and lay[2].n_items > 0 and lay[3].n_agg > 0
    elif name == "expand_mixed":
        assert len(lay) == 1
        n_pairs = lay[0].n_pairs
        assert n_pairs > 256 and n_pairs % 64 != 0
        bits = np.zeros(c.D.shape, np.int64)
        for i, j, cd, mask in code_masks(c.top, c.D):
            bits[:, (min(i, j) - c.top.pads) // 2] += mask
        in_list, cand = listed(c.top, c.D), has_candidate(c.D)
        assert {1, 2} == set(np.unique(bits[in_list]).tolist())  # 1- and 2-bit pairs mixed in the waves (clash rows: bit 0 alone)
        assert (cand & ~in_list).any() and (~cand).any()        # candidates the pair pass drops (kind == 0), and frames without the pair
        clash = ref["interaction"] == 0
        assert clash.sum() == c.top.K and (ref["min_distance"][clash] == 0.0).all() and (ref["max_distance"][clash] == 0.0).all()
    elif name == "capacity_1":
        assert lay[0].allocated and lay[0].cap == 1 and lay[0].grew and lay[0].n_agg == 0
        assert sum(ps.grew and ps.n_agg > 0 for ps in lay[1:]) >= 2
        _agg_only_rows(c, lay)
        assert not any(ps.grew for ps in c.layout(cap0=0))
    elif name == "capacity_exact":
        assert lay[0].allocated and lay[0].n_items == lay[0].cap == c.cap and not lay[0].grew
        assert lay[1].grew and lay[1].n_agg + lay[1].n_items == lay[1].cap + 1 and lay[1].n_agg > 0
        _agg_only_rows(c, lay)
        assert not any(ps.grew for ps in c.layout(cap0=0))
    elif name == "capacity_floor":
        assert c.cap == 0 and lay[0].allocated and lay[0].cap == CAP_FLOOR and lay[0].n_items < 100 and not lay[0].grew
        assert lay[1].n_items > CAP_FLOOR and lay[1].grew and lay[1].n_agg > 0
    elif name.startswith("key_bits_"):
        n = int(name.rsplit("_", 1)[1])
        assert c.top.n == n and len(lay) == 2
        assert ref["from_atom"][-1] == n - 1 and ref["from_atom"].max() == n - 1 and (ref["from_atom"][:-2] < n - 1).all()
        assert (np.diff(ref["from_atom"]) >= 0).all()
    elif name == "many_frames":
        assert c.chunk_atoms == 0 and [ps.frames for ps in lay] == [MAX_FRAMES_PER_PASS, c.F - MAX_FRAMES_PER_PASS]
        assert not any(ps.grew for ps in lay) and all(ps.skipped is None for ps in lay)
        assert ref["n_frames"].tolist() == [23334, 23334, 3]
    elif name.startswith("rounding_"):
        F = c.F
        assert sorted(set(ref["n_frames"].tolist())) == sorted({1, F - 1, F} - {0})
    else:
        raise AssertionError(f"no reach check for {name}")


def _agg_only_rows(c: Case, lay: list):
    """Rows that exist only in the aggregate when a later pass grows the buffers, and never appear again."""
    per = c.per
    masks = {r[:3]: r[3] for r in code_masks(c.top, c.D)}
    for p in (0, 1):
        keys = [k for k in masks if k[:2] == c.top.row(p) and masks[k].any()]
        assert keys
        for k in keys:
            last = int(np.flatnonzero(masks[k]).max()) // per
            assert any(ps.grew and ps.n_agg > 0 for ps in lay[last + 1:])
