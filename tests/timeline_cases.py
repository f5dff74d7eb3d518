"""Cases and references for contact timelines across frames (arp_contact_timelines: timeline.inl + the host half in table_ens.cpp).  No product
imports: tests/test_timeline_host.py checks the cases on the CPU (brute-force statistics == arp_timeline_stats, closed form == oracle loop, every
case reaches the boundary it is named for), tests/test_timeline_gpu.py runs them on the device.

Topology, frames and states are those of tests/freq_edge_cases.py (isolated two-atom motifs on the 1/256 A grid): freq_edge_cases.code_masks gives,
per (i, j, code), the boolean mask over the frames of a schedule D -- that mask IS the timeline of the row.  A motif is `present` in a frame at a
"one"- or "both"-band distance (one or two rows) and absent at APART.

References.
  brute(mask)           the statistics of one row from the definition: a plain Python loop over the frames.
  expected(top, D)      freq_edge_cases.reference(top, D) (the frequency table in closed form) + the five timeline columns from brute() + the packed
                        bitmap `timeline_words`, rows in the table's order.
  oracle_masks(top, D)  one oracle atomic_contacts call per frame, keeping the frame: {(i, j, code): mask}.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import freq_edge_cases as fe

STAT_COLUMNS = ["first_frame", "last_frame", "n_events", "longest_run", "mean_run"]
NONE = 0xFFFFFFFF
STEP_WORDS = 64  # words a wave of k_timeline_stats folds per step: a row of more than 2048 frames loops with a carried summary


def brute(mask) -> tuple:
    """(n_present, first, last, n_events, longest_run) of one row, bit by bit."""
    present, first, last, events, best, run = 0, NONE, NONE, 0, 0, 0
    for f, bit in enumerate(mask):
        if bit:
            if run == 0:
                events += 1
            run += 1
            present += 1
            if first == NONE:
                first = f
            last = f
            best = max(best, run)
        else:
            run = 0
    return present, first, last, events, best


def pack(masks: np.ndarray) -> np.ndarray:
    """bool [R, F] -> <u4 [R, ceil(F / 32)]: frame f is bit f & 31 of word f >> 5, the unused high bits of the last word are zero."""
    masks = np.asarray(masks, bool)
    R, F = masks.shape
    W = (F + 31) // 32
    padded = np.zeros((R, W * 32), bool)
    padded[:, :F] = masks
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(R, W, 32).astype(np.uint64) * weights).sum(2).astype("<u4")


def stat_columns(masks: np.ndarray) -> dict:
    """The five timeline columns + timeline_words of the rows whose masks are given (every row has at least one frame)."""
    masks = np.asarray(masks, bool)
    st = [brute(m) for m in masks]
    a = lambda k: np.array([s[k] for s in st], np.uint32)
    n, ev = a(0), a(3)
    assert (n > 0).all() if len(st) else True
    return {"first_frame": a(1), "last_frame": a(2), "n_events": ev, "longest_run": a(4),
            "mean_run": (n.astype(np.float64) / np.maximum(ev, 1).astype(np.float64)).astype(np.float32), "timeline_words": pack(masks)}


def row_masks(top: fe.Topology, D: np.ndarray) -> tuple:
    """([(i, j, code)], bool [R, F]) of the rows of the schedule's table, in its order."""
    rows = [r for r in fe.code_masks(top, D) if r[3].any()]
    F = np.asarray(D).shape[0]
    return [r[:3] for r in rows], (np.stack([r[3] for r in rows]) if rows else np.zeros((0, F), bool))


def expected(top: fe.Topology, D: np.ndarray) -> dict:
    out = fe.reference(top, D)
    keys, masks = row_masks(top, D)
    assert [(int(i), int(j), int(c)) for i, j, c in zip(out["from_atom"], out["to_atom"], out["interaction"])] == [tuple(map(int, k)) for k in keys]
    assert np.array_equal(masks.sum(1), out["n_frames"])
    out.update(stat_columns(masks))
    out["n_total_frames"] = int(np.asarray(D).shape[0])
    return out


def oracle_masks(top: fe.Topology, D: np.ndarray) -> dict:
    """fe.oracle_table's loop, keeping the frames: {(i, j, code): bool [F]}."""
    import oracle_binding as ob
    import synth

    xyz = fe.frames(top, D)
    atoms = synth.records_to_oracle(top.rec, flat=False)
    out = {}
    for f in range(xyz.shape[0]):
        atoms["x"], atoms["y"], atoms["z"] = xyz[f, :, 0], xyz[f, :, 1], xyz[f, :, 2]
        for q in ob.Structure.from_atoms(atoms, False).atomic_contacts("/", fe.VDW_COMP, fe.CUTOFF):
            kind = int(q["kind"])
            for c in range(len(ob.INTERACTIONS)):
                if kind >> c & 1:
                    out.setdefault((int(q["i"]), int(q["j"]), c), np.zeros(xyz.shape[0], bool))[f] = True
    return out


def assert_same(got: dict, want: dict, bitmap: bool = True):
    """Every frequency column (fe.assert_same_table), the five timeline columns and the whole bitmap for equality."""
    extra = STAT_COLUMNS + (["timeline_words", "n_total_frames"] if bitmap else [])
    assert set(got) == set(fe.COLUMNS) | set(extra), sorted(set(got) ^ (set(fe.COLUMNS) | set(extra)))
    fe.assert_same_table({c: got[c] for c in fe.COLUMNS}, {c: want[c] for c in fe.COLUMNS})
    for c in STAT_COLUMNS:
        assert got[c].dtype == want[c].dtype and np.array_equal(got[c].view(np.uint32), want[c].view(np.uint32)), (c, got[c], want[c])
    if bitmap:
        assert got["n_total_frames"] == want["n_total_frames"]
        assert got["timeline_words"].dtype == np.dtype("<u4") and got["timeline_words"].shape == want["timeline_words"].shape
        assert np.array_equal(got["timeline_words"], want["timeline_words"])


# ---- schedules -------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    top: fe.Topology
    D: np.ndarray
    per: int | None = None  # frames per pass (freq_chunk_atoms = per * n); None: the knob stays 0

    @property
    def F(self) -> int:
        return self.D.shape[0]

    @property
    def W(self) -> int:
        return (self.F + 31) // 32

    @property
    def chunk_atoms(self) -> int:
        return 0 if self.per is None else self.per * self.top.n

    def with_per(self, per: int | None) -> "Case":
        return Case(self.name, self.top, self.D, per)

    @property
    def per_frames(self) -> int:
        return fe.frames_per_pass(self.top.n, self.F, self.chunk_atoms)

    @property
    def n_passes(self) -> int:
        return -(-self.F // self.per_frames)

    def layout(self) -> list:
        return fe.layout(self.top, self.D, self.per_frames)


def runs_schedule(top: fe.Topology, F: int, runs: dict, states: dict | None = None) -> np.ndarray:
    """runs: motif -> [(first, last)] inclusive frame ranges in which it is present ("one" unless states[motif] says otherwise)."""
    D = fe.apart(F, top.K)
    for p, rr in runs.items():
        for a, b in rr:
            assert 0 <= a <= b < F
            fe.put(top, D, p, range(a, b + 1), (states or {}).get(p, "one"))
    return D


FRAME_COUNTS = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097]


def frame_count_case(F: int) -> Case:
    """Motif 0 in every frame (state "both": two rows), motif 1 in every other frame (events = ceil(F / 2)), motif 2 only in frame 0, motif 3 only
    in frame F - 1."""
    top = fe.topology(["CC", "ON", "OO", "CC"], "AB")
    D = fe.apart(F, top.K)
    fe.put(top, D, 0, range(F), "both")
    fe.put(top, D, 1, range(0, F, 2), "one")
    fe.put(top, D, 2, [0], "one")
    fe.put(top, D, 3, [F - 1], "one")
    return Case(f"frames_{F}", top, D)


BOUNDARY_F = 2100
BOUNDARY_RUNS = {
    0: [(20, 40)],                          # over 31 | 32
    1: [(32, 63)],                          # exactly word 1
    2: [(31, 64)],                          # one frame into both neighbours of word 1
    3: [(10, 20), (32, 127), (129, 140)],   # three whole words between partial neighbours
    4: [(2040, 2060)],                      # over 2047 | 2048: the 64-word step
    5: [(5, 14), (50, 52), (100, 109)],     # two equal longest runs
    6: [(0, 3), (BOUNDARY_F - 50, BOUNDARY_F - 1)],  # the longest run ends at F - 1, F % 32 != 0
    7: [(0, 9)],                            # "both" in [0, 9] and (below) "one" in [10, 19]: two rows of one atom pair with different timelines
    8: [(1990, BOUNDARY_F - 1)],            # whole words on both sides of the 64-word step
    9: [(0, BOUNDARY_F - 1)],               # every frame: all-ones words through both steps
}


def boundary_case() -> Case:
    top = fe.topology(["CC", "ON", "OO"] * 3 + ["CC"], "AB")
    D = runs_schedule(top, BOUNDARY_F, BOUNDARY_RUNS, {7: "both"})
    fe.put(top, D, 7, range(10, 20), "one")
    return Case("run_boundaries", top, D)


PASS_F = 69
PASS_SIZES = [5, 31, 32, 33, None]  # frames per pass; None: one pass


def pass_case(kind: str) -> Case:
    """gap: every motif is apart in frames 31 .. 65, so a whole pass in the middle has no pair for per = 31, 32, 33 (several for per = 5); rows only
    in the first pass, only in the last partial pass, and in both with the gap between.  dense: runs across every pass boundary."""
    top = fe.topology(["CC", "ON", "OO", "CC", "ON"], "BA")
    if kind == "gap":
        runs = {0: [(0, 2)], 1: [(67, 68)], 2: [(3, 8), (66, 68)], 3: [(0, 30), (66, 68)], 4: [(1, 1), (4, 4), (30, 30), (66, 66), (68, 68)]}
        states = {3: "both"}
    else:
        runs = {0: [(0, PASS_F - 1)], 1: [(f, f) for f in range(0, PASS_F, 2)], 2: [(28, 36)], 3: [(60, 67)], 4: [(4, 5), (30, 33), (61, 66)]}
        states = {0: "both"}
    return Case(f"passes_{kind}", top, runs_schedule(top, PASS_F, runs, states))


ROW_COUNTS = [(1, "AB", 0), (2, "BA", 0), (63, "AB", 0), (64, "BA", 2), (65, "AB", 3), (128, "BA", 0), (129, "BA", 5)]
ROW_F = 40


def row_count_case(R: int, order: str, pads: int) -> Case:
    """R motifs of one row each ("one"), each with its own timeline; "BA": the rows run (2p + 1, 2p); pads: lone atoms in front."""
    top = fe.topology((["CC", "ON", "OO"] * R)[:R], order, pads)
    D = fe.apart(ROW_F, top.K)
    for p in range(R):
        on = np.random.default_rng(1000 + p).random(ROW_F) < 0.4
        on[(11 * p) % ROW_F] = True
        fe.put(top, D, p, np.flatnonzero(on), "one")
    return Case(f"rows_{R}", top, D)


def mark_case() -> Case:
    """fe.expand_case: one pass whose pair list mixes pairs with 1 and 2 set bits, a partly filled tail wave, coincident atoms (code 0)."""
    c = fe.expand_case()
    return Case("mark_mixed", c.top, c.D, c.per)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = [frame_count_case(F) for F in FRAME_COUNTS]
    out += [boundary_case(), pass_case("gap"), pass_case("dense"), mark_case()]
    out += [row_count_case(*rc) for rc in ROW_COUNTS]
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def expected_of(name: str) -> dict:
    c = cases()[name]
    return expected(c.top, c.D)


def _runs_of(mask) -> list:
    """[(first, last)] of the maximal runs of a mask."""
    m = np.concatenate([[False], np.asarray(mask, bool), [False]])
    d = np.diff(m.astype(np.int8))
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


def check_reach(name: str):
    """The precondition of a case: its schedule reaches the boundary it is named for (word, step, pass and row counts computed from the schedule).
    Asserted by the host test, and again by the GPU test before it calls the device."""
    c = cases()[name]
    want = expected_of(name)
    keys, masks = row_masks(c.top, c.D)
    R, F = masks.shape
    assert c.per_frames * c.top.n < 300000
    if name.startswith("frames_"):
        assert c.n_passes == 1 and R == 5 and c.W == -(-F // 32)
        assert (c.W > STEP_WORDS) == (F > 2048) and (F % 32 == 0) == (F in (32, 64, 2048))
        by_motif = {(min(i, j)) // 2: k for k, (i, j, _) in enumerate(keys)}  # (the last row of each motif)
        assert want["n_events"][by_motif[1]] == -(-F // 2) and want["n_frames"][by_motif[1]] == -(-F // 2)
        assert want["n_frames"][by_motif[0]] == F and want["longest_run"][by_motif[0]] == F and want["n_events"][by_motif[0]] == 1
        assert (want["first_frame"][by_motif[2]], want["last_frame"][by_motif[2]]) == (0, 0)
        assert (want["first_frame"][by_motif[3]], want["last_frame"][by_motif[3]]) == (F - 1, F - 1)
        if F % 32:
            assert (want["timeline_words"][:, -1] >> np.uint32(F % 32) == 0).all()
    elif name == "run_boundaries":
        assert F % 32 != 0 and c.W > STEP_WORDS and c.n_passes == 1
        runs = {}
        for (i, j, code), m in zip(keys, masks):
            runs.setdefault((min(i, j) // 2, code), _runs_of(m))
        one = lambda p: runs[(p, fe.BANDS[c.top.kinds[p]]["one"][2][0])]
        assert one(0) == [(20, 40)] and one(1) == [(32, 63)] and one(2) == [(31, 64)]
        assert one(3) == [(10, 20), (32, 127), (129, 140)]
        a, b = one(4)[0]
        assert a < 2048 <= b and 2048 == STEP_WORDS * 32
        lens = [b - a + 1 for a, b in one(5)]
        assert sorted(lens)[-2:] == [10, 10] and len(lens) == 3
        assert one(6)[-1] == (F - 50, F - 1) and max(b - a + 1 for a, b in one(6)) == 50
        assert c.top.kinds[7] == "ON" and runs[(7, 3)] == [(0, 9)] and runs[(7, 4)] == [(0, 19)]  # two rows of one atom pair
        a, b = one(8)[0]
        assert a // 32 + 1 < 2048 // 32 < b // 32  # whole words on both sides of the step
        assert one(9) == [(0, F - 1)]
    elif name.startswith("passes_"):
        assert PASS_F % 5 and PASS_F % 31 and PASS_F % 32 and PASS_F % 33
        for per, n_passes in zip(PASS_SIZES, (14, 3, 3, 3, 1)):
            cc = c.with_per(per)
            assert cc.n_passes == n_passes and (per is None or cc.per_frames == per)
            lay = cc.layout()
            assert len(lay) == n_passes and (per is None or lay[-1].frames == PASS_F % per)
            skipped = [ps.skipped is not None for ps in lay]
            if name == "passes_gap" and per is not None:
                assert any(skipped[1:-1]) and not skipped[0] and not skipped[-1]
                last0 = lay[-1].f0
                only_first = [m[:lay[0].frames].any() and not m[lay[0].frames:].any() for m in masks]
                only_last = [m[last0:].any() and not m[:last0].any() for m in masks]
                gap = [m[:lay[0].frames].any() and m[last0:].any() and not m[lay[1].f0:lay[1].f0 + lay[1].frames].any() for m in masks]
                assert any(only_first) and any(only_last) and any(gap)
            if name == "passes_dense" and per is not None:
                assert not any(skipped)
                bounds = [ps.f0 for ps in lay[1:]]
                assert all(any(m[b - 1] and m[b] for m in masks) for b in bounds)  # a run continues across every pass boundary
                if per % 32:
                    assert any(b // 32 == (b - 1) // 32 for b in bounds)  # two passes share a word
    elif name.startswith("rows_"):
        want_R = int(name.split("_")[1])
        assert R == want_R == c.top.K and c.n_passes == 1
        assert len({m.tobytes() for m in masks}) == R  # a timeline of its own per row
        order = [rc for rc in ROW_COUNTS if rc[0] == want_R][0]
        assert (c.top.order, c.top.pads) == order[1:]
        if c.top.order == "BA":
            assert all(i == j + 1 for i, j, _ in keys)
    elif name == "mark_mixed":
        fe.check_reach("expand_mixed")
        assert (want["interaction"] == 0).sum() == c.top.K
    else:
        raise AssertionError(f"no reach check for {name}")
