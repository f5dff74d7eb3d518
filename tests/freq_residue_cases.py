"""Built cases and references for residue-level contact frequencies across frames (arp_residue_contact_frequencies: the residue mode of freq.inl +
the host half in table_ens.cpp).  No product imports: tests/test_freq_residue_host.py checks the cases on the CPU (closed form
== oracle loop, every case reaches the edge it is named for), tests/test_freq_residue_gpu.py runs them on the device.

Topology.  The two-atom motifs of tests/freq_edge_cases.py (same places, same 1/256 A grid, so every distance is exact in f32 and compared for
equality), grouped into FAT residue pairs: the chain-A atoms of the motifs of group g are one residue (chain A, resi g + 1) and their chain-B
atoms are one residue (chain B, resi g + 1) -- the pdbtbx-like hierarchy builder files atoms of one (chain, resi, insertion) under one residue.
All motifs of a group are of one kind (a residue has one name).  Motifs stay 32 A apart, so the only pairs are a motif's own: one (residue pair,
frame) holds as many items per code as the group has motifs in the code's bands.  Lone atoms in front are residues of their own (chain A, resi
1001 ...).  Residue ordinals run in order of first appearance in the file.

Bands.  freq_edge_cases.BANDS, unchanged; the oracle loop of the host test pins them again on fat residues -- the bands in use here are CC both
[2.5, 3.5] (codes 3 + 18) and one [3.75, 4.375] (18), ON both [2.5, 3.25] (3 + 4) and one [3.3125, 4.0] (4), OO one [3.25, 3.5] (7), and the
states 5.5 A (a candidate without a code), 8.0 A (no pair) -- every case's closed form equals the oracle loop exactly, so a motif's codes do not
depend on what else its residue holds.

References.
  reference(case)       (a) closed form from the schedule: per (residue pair, code) the frames in which ANY motif of the group has the code, per
                        such frame the smallest distance among those motifs (c_f), then count, min c_f, max c_f; rows ordered by (A, B, code).
  oracle_table(case)    (b) one oracle atomic_contacts call per frame, grouped by residue in numpy (per frame first, then over frames).
  layout(case, ...)     (c) what the device pipeline does pass by pass: frames per pass (pass size, frame cap 2^fb - 1), pairs, items, buffer
                        growth, the (row, tag) sub-runs of the sorted items (first reduction) and the rows over the sub-run entries (second).
"""
from __future__ import annotations

import functools
import types
from dataclasses import dataclass, field

import numpy as np

import freq_edge_cases as ec

FRAME_BITS_MAX, CODE_BITS = 17, 5
COLUMNS = ["interaction", "from_chain", "from_resn", "from_resi", "from_insertion", "to_chain", "to_resn", "to_resi", "to_insertion", "n_frames", "frequency",
           "min_distance", "max_distance", "from_residue", "to_residue"]


def fat_topology(groups, order: str = "AB", pads: int = 0):
    """groups: [(kind, motifs)] -> (ec.Topology with the residues regrouped, group [K]: the fat pair of every motif)."""
    kinds, group = [], []
    for g, (kind, size) in enumerate(groups):
        kinds += [kind] * size
        group += [g] * size
    top = ec.topology(kinds, order, pads)
    rec = {k: v.copy() for k, v in top.rec.items()}
    rec["resi"][:pads] = 1001 + np.arange(pads)
    for p, g in enumerate(group):
        rec["resi"][top.fixed(p)] = rec["resi"][top.moving(p)] = g + 1
    return ec.Topology(top.kinds, order, pads, rec), np.array(group, np.int64)


def residues(rec: dict):
    """(res [n]: the residue ordinal of every atom, first [n_res]: the first atom of every residue), ordinals in order of first appearance."""
    seen, res, first = {}, [], []
    for k in range(len(rec["x"])):
        key = (bytes(rec["chain"][k]), int(rec["resi"][k]), bytes(rec["icode"][k]))
        if key not in seen:
            seen[key] = len(seen)
            first.append(k)
        res.append(seen[key])
    return np.array(res, np.int64), np.array(first, np.int64)


@dataclass
class Case:
    name: str
    top: ec.Topology
    group: np.ndarray
    D: np.ndarray
    per: int | None = None   # frames per pass through freq_chunk_atoms = per * n; None: the knob stays 0
    cap: int = 0             # freq_cap_items
    frame_bits: int = 0      # freq_frame_bits
    oracle_frames: np.ndarray | None = None

    @property
    def F(self) -> int:
        return self.D.shape[0]

    @property
    def chunk_atoms(self) -> int:
        return 0 if self.per is None else self.per * self.top.n

    def frames(self) -> np.ndarray:
        return ec.frames(self.top, self.D)


def frame_bits(n_res: int, knob: int = 0) -> int:
    rb = 1
    while rb < 29 and (1 << rb) < n_res:
        rb += 1
    fb = min(FRAME_BITS_MAX, 64 - CODE_BITS - 2 * rb)
    return min(fb, knob) if knob else fb


def frames_per_pass(case: Case, chunk_atoms: int | None = None, knob: int | None = None) -> int:
    n_res = int(residues(case.top.rec)[0].max()) + 1
    fb = frame_bits(n_res, case.frame_bits if knob is None else knob)
    return min(ec.frames_per_pass(case.top.n, case.F, case.chunk_atoms if chunk_atoms is None else chunk_atoms), (1 << fb) - 1)


def row_items(case: Case, D: np.ndarray | None = None):
    """keys [(A, B, code)] sorted, cnt [rows, F] items of the row per frame, cf [rows, F] f32 closest approach per frame (inf: none)."""
    D = case.D if D is None else D
    res, _ = residues(case.top.rec)
    acc = {}
    for i, j, c, mask in ec.code_masks(case.top, D):
        if not mask.any():
            continue
        p = (min(i, j) - case.top.pads) // 2
        cnt, cf = acc.setdefault((int(res[i]), int(res[j]), c), (np.zeros(D.shape[0], np.int64), np.full(D.shape[0], np.inf, np.float32)))
        cnt += mask
        cf[mask] = np.minimum(cf[mask], D[mask, p].astype(np.float32))
    keys = sorted(acc)
    F = D.shape[0]
    return keys, (np.stack([acc[k][0] for k in keys]) if keys else np.zeros((0, F), np.int64)), (np.stack([acc[k][1] for k in keys]) if keys else np.zeros((0, F), np.float32))


def _table(case: Case, F: int, rows: list) -> dict:
    """rows: [(A, B, code, count, f32 min, f32 max)] in (A, B, code) order -> the columns of the residue frequency table."""
    rec = case.top.rec
    _, first = residues(rec)
    a = lambda k, dt: np.array([r[k] for r in rows], dtype=dt)
    A, B, cnt = a(0, np.int64), a(1, np.int64), a(3, np.uint32)
    out = {"interaction": a(2, np.int32), "from_residue": A.astype(np.int32), "to_residue": B.astype(np.int32), "n_frames": cnt,
           "frequency": (cnt.astype(np.float64) / float(F)).astype(np.float32), "min_distance": a(4, np.float32), "max_distance": a(5, np.float32)}
    for side, idx in (("from", first[A] if len(rows) else A), ("to", first[B] if len(rows) else B)):
        out[f"{side}_chain"] = rec["chain"][idx]
        out[f"{side}_resn"] = rec["resn"][idx]
        out[f"{side}_resi"] = rec["resi"][idx]
        out[f"{side}_insertion"] = rec["icode"][idx]
    return out


def reference(case: Case, D: np.ndarray | None = None) -> dict:
    """(a) the residue frequency table in closed form from the schedule."""
    D = case.D if D is None else D
    keys, cnt, cf = row_items(case, D)
    rows = []
    for k, key in enumerate(keys):
        on = cnt[k] > 0
        rows.append(key + (int(on.sum()), cf[k][on].min(), cf[k][on].max()))
    return _table(case, D.shape[0], rows)


def oracle_table(case: Case, D: np.ndarray | None = None) -> dict:
    """(b) one oracle atomic_contacts call per frame; per frame the smallest distance of every (residue, residue, code), then over the frames."""
    import oracle_binding as ob
    import synth

    D = case.D if D is None else D
    xyz = ec.frames(case.top, D)
    res, _ = residues(case.top.rec)
    atoms = synth.records_to_oracle(case.top.rec, flat=False)
    agg = {}
    for f in range(xyz.shape[0]):
        atoms["x"], atoms["y"], atoms["z"] = xyz[f, :, 0], xyz[f, :, 1], xyz[f, :, 2]
        here = {}
        for q in ob.Structure.from_atoms(atoms, False).atomic_contacts("/", ec.VDW_COMP, ec.CUTOFF):
            d, kind = np.float32(q["dist"]), int(q["kind"])
            for c in range(len(ob.INTERACTIONS)):
                if kind >> c & 1:
                    key = (int(res[int(q["i"])]), int(res[int(q["j"])]), c)
                    here[key] = min(here.get(key, d), d)
        for key, d in here.items():
            n, mn, mx = agg.get(key, (0, d, d))
            agg[key] = (n + 1, min(mn, d), max(mx, d))
    return _table(case, xyz.shape[0], [k + agg[k] for k in sorted(agg)])


def assert_same_table(got: dict, want: dict):
    """Every column, row order included, for exact equality (strings compared at the reference's width; floats by their bits)."""
    assert set(got) == set(COLUMNS) and set(want) == set(COLUMNS), (sorted(got), sorted(want))
    for c in COLUMNS:
        assert len(got[c]) == len(want[c]), (c, len(got[c]), len(want[c]))
        g = got[c].astype(want[c].dtype) if want[c].dtype.kind == "S" else got[c]
        if want[c].dtype.kind == "f":
            assert g.dtype == np.float32, c
            assert np.array_equal(g.view(np.uint32), want[c].astype(np.float32).view(np.uint32)), (c, g, want[c])
        else:
            assert np.array_equal(g, want[c].astype(g.dtype)), (c, g, want[c])


# ---- (c) the layout the device pipeline must produce -----------------------------------------------------------------------------------------
@dataclass
class Pass:
    f0: int
    frames: int
    n_pairs: int
    n_items: int
    n_agg: int           # residue rows of the aggregate before the pass
    skipped: bool        # no listed pair: the host loop goes on to the next pass
    cap: int
    grew: bool
    sub: list = field(default_factory=list)   # first reduction: ec.Run((row, tag), start, length, tag == 0) over the sorted items
    rows: list = field(default_factory=list)  # second reduction: ec.Run(row, start, length, has an aggregate entry) over the sub-run entries

    @property
    def m(self) -> int:
        return self.n_agg + self.n_items

    def edges(self, which: str) -> set:
        runs = self.sub if which == "sub" else self.rows
        return ec.run_edges(types.SimpleNamespace(m=(runs[-1].end + 1) if runs else 0, runs=runs))


def layout(case: Case, per: int | None = None, cap0: int | None = None) -> list:
    per = frames_per_pass(case) if per is None else per
    cap0 = case.cap if cap0 is None else cap0
    keys, cnt, _ = row_items(case)
    pairs = ec.listed(case.top, case.D)
    in_agg = np.zeros(len(keys), bool)
    cap, out = 0, []
    for f0 in range(0, case.F, per):
        fc = min(per, case.F - f0)
        here = cnt[:, f0:f0 + fc]
        ps = Pass(f0, fc, int(pairs[f0:f0 + fc].sum()), int(here.sum()), int(in_agg.sum()), False, cap, False)
        out.append(ps)
        if ps.n_pairs == 0:
            ps.skipped = True
            continue
        if cap == 0:
            cap = cap0 if cap0 > 0 else max(ec.CAP_FLOOR, 2 * ps.n_pairs)
            ps.cap = cap
        if ps.m > cap:
            cap = ps.m + ps.m // 4
            ps.grew = True
        at = entry = 0
        for k in np.flatnonzero(in_agg | (here.sum(1) > 0)):
            start_entry = entry
            if in_agg[k]:
                ps.sub.append(ec.Run((keys[k], 0), at, 1, True))
                at, entry = at + 1, entry + 1
            for t in np.flatnonzero(here[k]):
                ps.sub.append(ec.Run((keys[k], int(t) + 1), at, int(here[k, t]), False))
                at, entry = at + int(here[k, t]), entry + 1
            ps.rows.append(ec.Run(keys[k], start_entry, entry - start_entry, bool(in_agg[k])))
        assert at == ps.m
        in_agg |= here.sum(1) > 0
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
def _on(case_top, D, group, g, frames, members, state):
    """The motifs `members` (positions inside group g) of group g in the frames `frames`: state "both" / "one" (distances varied) or a distance."""
    ps = np.flatnonzero(group == g)[np.asarray(members, np.int64)]
    for p in ps:
        if isinstance(state, str):
            ec.put(case_top, D, int(p), frames, state)
        else:
            D[np.asarray(frames, np.int64), p] = state


def semantics_case() -> Case:
    """What a residue row means, on the smallest shapes:
      group 0 (CC x 4)  dedup: all four motifs in the one-code band in frames 0 and 3, two of them in frame 5 -> code 18 has n_frames 3, not 10
      group 1 (CC x 2)  union: motif 0 on even frames, motif 1 on odd frames -> the atom table says 0.5 and 0.5, the residue row 1.0
      group 2 (CC x 2)  closest approach: frame 1 holds {3.0, 4.25}, frame 4 holds {3.5} -> code 18 has min 3.0 and max 3.5, not 4.25
      group 3 (ON x 2)  codes kept apart: in frames 2 and 6 motif 0 is in the two-code band (3 + 4) and motif 1 in the one-code band (4)
      group 4 (OO x 1)  a thin pair next to the fat ones; group 5 (CC x 3) never in contact: no row"""
    top, group = fat_topology([("CC", 4), ("CC", 2), ("CC", 2), ("ON", 2), ("OO", 1), ("CC", 3)], "AB", pads=2)
    F = 8
    D = ec.apart(F, top.K)
    _on(top, D, group, 0, [0, 3], [0, 1, 2, 3], "one")
    _on(top, D, group, 0, [5], [1, 3], "one")
    _on(top, D, group, 1, range(0, F, 2), [0], "one")
    _on(top, D, group, 1, range(1, F, 2), [1], "one")
    _on(top, D, group, 2, [1], [0], 3.0)
    _on(top, D, group, 2, [1], [1], 4.25)
    _on(top, D, group, 2, [4], [1], 3.5)
    _on(top, D, group, 3, [2, 6], [0], "both")
    _on(top, D, group, 3, [2, 6], [1], "one")
    _on(top, D, group, 4, [0, 7], [0], "one")
    _on(top, D, group, 5, [3], [0, 1], ec.K0)
    return Case("semantics", top, group, D)


SUB_F = 80


def subrun_case(second_pass: bool) -> Case:
    """One pass whose sorted items form (row, frame) sub-runs at chosen lanes.  Group 0 (OO x 65, one code) is on with 64, 65, 62, 1, 1, 65, 10
    motifs in frames 0 .. 6: sub-runs [0, 64) [64, 129) [129, 191) [191] [192] [193, 258) [258, 268) -- a sub-run of 64 from lane 0, one of 65, a
    single item at lane 63 and one at lane 0, one across sorted position 255 -> 256, and a row whose sub-runs span more than three waves.  Group
    1 (ON x 3) has two codes per item; group 2 (CC x 2) is on in 70 frames: a row of 70 entries for the second reduction.  second_pass: SUB_F
    more frames in front in which groups 0 and 2 are on once, so that their rows carry the aggregate's entry (tag 0) in front of their sub-runs
    and every position moves by one."""
    top, group = fat_topology([("OO", 65), ("ON", 3), ("CC", 2)], "AB")
    F = SUB_F
    off = F if second_pass else 0
    D = ec.apart(off + F, top.K)
    for f, count in enumerate([64, 65, 62, 1, 1, 65, 10]):
        _on(top, D, group, 0, [off + f], [(7 * f + k) % 65 for k in range(count)], "one")
    _on(top, D, group, 1, [off + 2, off + 9], [0, 1, 2], "both")
    _on(top, D, group, 1, [off + 3], [1], "one")
    _on(top, D, group, 2, off + np.arange(5, 75), [0], "one")
    _on(top, D, group, 2, off + np.arange(5, 75, 2), [1], "both")
    if second_pass:
        _on(top, D, group, 0, [11], [3, 4], "one")
        _on(top, D, group, 2, [40], [1], "one")
    return Case("subruns_second_pass" if second_pass else "subruns", top, group, D, per=F)


def pass_case(name: str, per: int | None, cap: int = 0, frame_bits: int = 0) -> Case:
    """22 frames in passes of 4 (the last of 2): pass 0 and pass 2 have no pair at all (a pass without pairs in front and in the middle).
      group 0 (CC x 3)  on in frame 5, in frame 15 (the last of pass 3) and in frame 16 (the first of pass 4, another motif, closer)
      group 1 (ON x 2)  only in pass 1: from then on its rows live in the aggregate alone
      group 2 (OO x 2)  first in pass 4: new keys beside an aggregate
      group 3 (CC x 2)  in passes 1, 3, 4 and 5, the two motifs taking turns; group 4 (ON x 1) in frames 7 and 19 .. 21
      group 5 (CC x 6)  all six motifs in the two-code band in frames 16 .. 21: passes 4 and 5 hold many more items than the passes before them
                        (with freq_cap_items = 1 the buffers grow once without and once with an aggregate to keep)
    With freq_frame_bits = 2 the same frames run 3 to a pass: frames 15 and 16 then share pass 5 and frames 5 | 6, 14 | 15, 17 | 18 straddle."""
    top, group = fat_topology([("CC", 3), ("ON", 2), ("OO", 2), ("CC", 2), ("ON", 1), ("CC", 6)], "BA", pads=1)
    F = 22
    D = ec.apart(F, top.K)
    _on(top, D, group, 0, [5], [0, 1], "both")
    _on(top, D, group, 0, [15], [2], 4.0)
    _on(top, D, group, 0, [16], [0], 3.75)
    _on(top, D, group, 1, [4, 6], [0, 1], "both")
    _on(top, D, group, 1, [7], [1], "one")
    _on(top, D, group, 2, [17, 18, 21], [0], "one")
    _on(top, D, group, 2, [18], [1], "one")
    _on(top, D, group, 3, [4, 6, 12, 14, 16, 18, 20], [0], "one")
    _on(top, D, group, 3, [5, 6, 13, 14, 17, 18, 21], [1], "both")
    _on(top, D, group, 4, [7, 19, 20, 21], [0], "one")
    _on(top, D, group, 5, range(16, F), range(6), "both")
    return Case(name, top, group, D, per=per, cap=cap, frame_bits=frame_bits)


def many_frames_case() -> Case:
    """70 000 frames of a four-atom topology (one fat pair of two CC motifs): two passes under the cap of 65 535 frames per pass.  Motif 0 is
    on when f % 3 == 0; motif 1 in frames 65 534 (the last of pass 0), 65 535 (the first of pass 1: also motif 0's) and 69 999 (also motif 0's)."""
    F = 70000
    top, group = fat_topology([("CC", 2)], "AB")
    D = ec.apart(F, top.K)
    _on(top, D, group, 0, range(0, F, 3), [0], "both")
    _on(top, D, group, 0, [65534, 65535, 69999], [1], "one")
    sub = sorted({0, F - 1, ec.MAX_FRAMES_PER_PASS - 1, ec.MAX_FRAMES_PER_PASS} | set(range(0, F, 997)))
    return Case("many_frames", top, group, D, oracle_frames=np.array(sub))


def trivial_case(name: str) -> Case:
    top, group = fat_topology([("CC", 2), ("ON", 2)], "AB")
    if name == "one_frame":
        D = ec.apart(1, top.K)
        _on(top, D, group, 0, [0], [0, 1], "both")
        _on(top, D, group, 1, [0], [1], "one")
    else:  # "no_contact": candidates without a code, and frames without any pair
        D = ec.apart(3, top.K)
        D[1] = ec.K0
    return Case(name, top, group, D)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = [semantics_case(), subrun_case(False), subrun_case(True), pass_case("passes", 4), pass_case("passes_cap1", 4, cap=1),
           pass_case("passes_frame_bits2", None, frame_bits=2), many_frames_case(), trivial_case("one_frame"), trivial_case("no_contact")]
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def reference_of(name: str) -> dict:
    return reference(cases()[name])


def _row(ref: dict, A: int, B: int, code: int) -> int:
    k = np.flatnonzero((ref["from_residue"] == A) & (ref["to_residue"] == B) & (ref["interaction"] == code))
    assert len(k) == 1, (A, B, code)
    return int(k[0])


def pair_of(case: Case, g: int) -> tuple:
    """(A, B): the residue ordinals of fat pair g, from the chain-A residue to the chain-B residue."""
    res, _ = residues(case.top.rec)
    i, j = case.top.row(int(np.flatnonzero(case.group == g)[0]))
    return int(res[i]), int(res[j])


def check_reach(name: str):
    """The precondition of a case: schedule and layout reach what the case is named for.  Asserted by the host test, and again by the GPU test
    before it calls the device."""
    c = cases()[name]
    ref = reference_of(name)
    lay = layout(c)
    res, first = residues(c.top.rec)
    assert (np.diff(first) > 0).all() and len(first) == c.top.pads + 2 * (int(c.group.max()) + 1)  # fat residues: fewer residues than atoms
    assert c.top.n * max(ps.frames for ps in lay) < 300000 or name == "many_frames"
    if name == "semantics":
        assert len(lay) == 1 and not lay[0].skipped
        keys, cnt, cf = row_items(c)
        r = lambda g, code: keys.index(pair_of(c, g) + (code,))
        assert cnt[r(0, 18)].tolist() == [4, 0, 0, 4, 0, 2, 0, 0] and ref["n_frames"][_row(ref, *pair_of(c, 0), 18)] == 3
        k = _row(ref, *pair_of(c, 1), 18)
        assert (cnt[r(1, 18)] == 1).all() and ref["n_frames"][k] == c.F and ref["frequency"][k] == np.float32(1.0)
        atom_rows = [m for _, _, code, m in ec.code_masks(c.top, c.D) if code == 18 and m.sum() == c.F // 2]
        assert len(atom_rows) >= 2  # the atom table's 0.5 and 0.5
        k = _row(ref, *pair_of(c, 2), 18)
        assert cnt[r(2, 18)].tolist() == [0, 2, 0, 0, 1, 0, 0, 0]
        assert (ref["min_distance"][k], ref["max_distance"][k], ref["n_frames"][k]) == (np.float32(3.0), np.float32(3.5), 2)
        assert 4.25 in c.D[1]  # what the maximum over all items would be
        assert cnt[r(3, 3)].tolist() == [0, 0, 1, 0, 0, 0, 1, 0] and cnt[r(3, 4)].tolist() == [0, 0, 2, 0, 0, 0, 2, 0]
        assert not any(key[:2] == pair_of(c, 5) for key in keys)
        assert max(ps_run.length for ps_run in lay[0].sub) == 4
    elif name.startswith("subruns"):
        second = name.endswith("second_pass")
        assert len(lay) == (2 if second else 1) and not any(ps.grew or ps.skipped for ps in lay)
        ps = lay[-1]
        sub0 = [r for r in ps.sub if r.key[0][:2] == pair_of(c, 0)]
        shift = 1 if second else 0
        assert [(r.start, r.length) for r in sub0 if r.key[1]] == [(s + shift, n) for s, n in ((0, 64), (64, 65), (129, 62), (191, 1), (192, 1), (193, 65), (258, 10))]
        assert second == (sub0[0].key[1] == 0) and (ps.n_agg > 0) == second
        edges = ps.edges("sub")
        if not second:
            assert {"run64_at_lane0", "run65_at_lane0", "single_at_lane63", "single_at_lane0", "run_across_255_256", "ragged_tail"} <= edges, edges
        else:
            assert {"run64_at_lane1", "single_at_lane0", "run_across_255_256"} <= edges, edges
            assert any(r.in_agg for r in ps.rows) and any(not r.in_agg for r in ps.rows)
        assert (sub0[-1].end // 64) - (sub0[0].start // 64) >= 3  # one row's sub-runs over more than three waves
        assert any(r.length == 70 + shift for r in ps.rows) and any(r.start // 64 != r.end // 64 for r in ps.rows)  # second reduction: a row across waves
        assert len({r.key[0][2] for r in ps.sub if r.key[0][:2] == pair_of(c, 1)}) == 2
    elif name.startswith("passes"):
        if name == "passes_frame_bits2":
            assert c.chunk_atoms == 0 and [ps.frames for ps in lay] == [3] * 7 + [1] and frames_per_pass(c, knob=0) == c.F
            assert max(r.key[1] for ps in lay for r in ps.sub) == 3  # the largest tag the two bits hold
            assert lay[0].skipped and sum(ps.skipped for ps in lay) >= 2
            tags = {(ps.f0, r.key[1]) for ps in lay for r in ps.sub if r.key[0][:2] == pair_of(c, 3)}
            assert {(3, 3), (6, 1)} <= tags  # frames 5 | 6: the last tag of one pass, the first of the next
            return
        assert [ps.frames for ps in lay] == [4] * 5 + [2] and [ps.skipped for ps in lay] == [True, False, True, False, False, False]
        p3, p4 = lay[3], lay[4]
        g0 = pair_of(c, 0)
        assert any(r.key == (g0 + (18,), 4) for r in p3.sub) and any(r.key == (g0 + (18,), 1) for r in p4.sub) and any(r.key == (g0 + (18,), 0) for r in p4.sub)
        in_agg_only = [r for r in p4.rows if r.in_agg and r.length == 1]
        new = [r for r in p4.rows if not r.in_agg]
        both = [r for r in p4.rows if r.in_agg and r.length > 1]
        assert in_agg_only and new and both
        assert any(r.key[:2] == pair_of(c, 1) for r in in_agg_only) and {r.key[:2] for r in new} == {pair_of(c, 2), pair_of(c, 5)}
        k = _row(ref, *g0, 18)
        assert (ref["n_frames"][k], ref["min_distance"][k], ref["max_distance"][k]) == (3, np.float32(c.D[5, :3].min()), np.float32(4.0))
        if name == "passes_cap1":
            assert lay[1].cap == 1 and lay[1].grew and lay[1].n_agg == 0 and [ps.grew and ps.n_agg > 0 for ps in lay] == [False, False, False, False, True, False]
            assert not any(ps.grew for ps in layout(c, cap0=0))
    elif name == "many_frames":
        assert c.chunk_atoms == 0 and [ps.frames for ps in lay] == [ec.MAX_FRAMES_PER_PASS, c.F - ec.MAX_FRAMES_PER_PASS]
        assert not any(ps.grew or ps.skipped for ps in lay)
        assert ref["interaction"].tolist() == [3, 18] and ref["n_frames"].tolist() == [23334, 23335]
        assert max(r.key[1] for r in lay[0].sub) == ec.MAX_FRAMES_PER_PASS and any(r.key[1] == 1 and r.length == 2 for r in lay[1].sub)
    elif name == "one_frame":
        assert c.F == 1 and len(ref["n_frames"]) == 3 and (ref["n_frames"] == 1).all() and (ref["frequency"] == 1.0).all()
        assert np.array_equal(ref["min_distance"], ref["max_distance"])
    elif name == "no_contact":
        assert all(ps.skipped for ps in lay) and all(len(ref[col]) == 0 for col in COLUMNS) and ec.has_candidate(c.D).any()
    else:
        raise AssertionError(f"no reach check for {name}")


# ---- ring items (ARP_FREQ_RINGS): the motifs of tests/freq_ring_cases.py by residue -------------------------------------------------------------
def ring_reference(case) -> dict:
    """The closed-form ring rows of a freq_ring_cases.Case by residue, ordered by (A, B, code).  The chain-A residue of motif p is ordinal p, its
    partner ordinal K + pads + p (file order: chain A's residues, the lone atoms, the partners).  An "alt" motif's two ring entities are one
    residue: its hits give ONE row with the motif's count; "rc" rows run from the ring's residue to the LYS; distances are the schedule's (f64:
    the device's are f32 from fitted planes, so they are compared within the project's 1e-5, not for equality)."""
    import freq_ring_cases as rg

    K = len(case.kinds)
    rows = []
    for p, kind in enumerate(case.kinds):
        hits = {}
        for f in range(case.F):
            st = case.state(f, p)
            code, dist = (st[2], st[0]) if kind == "rc" else (st[3], st[2])
            if code is not None:
                hits.setdefault(rg.CODES[code], []).append(dist)
        for code, d in hits.items():
            rows.append((p, K + case.pads + p, code, len(d), min(d), max(d)))
    rows.sort()
    a = lambda k, dt: np.array([r[k] for r in rows], dtype=dt)
    return {"from_residue": a(0, np.int32), "to_residue": a(1, np.int32), "interaction": a(2, np.int32), "n_frames": a(3, np.uint32),
            "frequency": (a(3, np.float64) / case.F).astype(np.float32), "min_distance": a(4, np.float64), "max_distance": a(5, np.float64)}
