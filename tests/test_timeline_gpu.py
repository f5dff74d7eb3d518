"""Contact timelines across frames (arp_contact_timelines) on the device.

Built cases (tests/timeline_cases.py) compare every column and the whole bitmap with the closed form of the schedule, after asserting that the
case reaches the boundary it is named for; tests/test_timeline_host.py pins the closed form to the oracle on the CPU.  Natural inputs are compared
with the timeline by definition -- one Context.atomic_contacts call per frame and, with rings, one Context.get_contacts call per frame, keeping
the frame -- and, column by column, with the frequency call on the same arguments.  Expected values never come from the timeline call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import arpeggia_amd as aa
import freq_common as fcm
import freq_edge_cases as fe
import freq_residue_common as fc
import freq_ring_cases as rg
import synth
import timeline_cases as tc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib

pytestmark = pytest.mark.gpu

KNOBS = ("freq_chunk_atoms", "freq_cap_items", "freq_frame_bits", "timeline_cap_bytes")


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


def to_bytes(t: dict) -> bytes:
    return b"".join(np.ascontiguousarray(t[c]).tobytes() for c in sorted(t))


def run(ctx, c: tc.Case, **kw) -> dict:
    s = aa.Structure.from_records(c.top.rec)
    assert s.n_atoms == c.top.n
    aa.debug_set("freq_chunk_atoms", c.chunk_atoms)
    return ctx.contact_timelines(s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF, **kw)


def check(ctx, name: str) -> dict:
    tc.check_reach(name)
    got = run(ctx, tc.cases()[name])
    tc.assert_same(got, tc.expected_of(name))
    return got


# ---- closed-form cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", tc.FRAME_COUNTS)
def test_frame_counts(ctx, F):
    """One word, a word and a bit, 64 words, the 64-word step and two steps: a contact in every frame, in every other frame (events = ceil(F / 2)),
    only in frame 0, only in frame F - 1."""
    got = check(ctx, f"frames_{F}")
    assert got["timeline_words"].shape == (5, (F + 31) // 32) and got["n_total_frames"] == F
    assert sorted(got["n_events"].tolist())[-1] == -(-F // 2)


def test_run_boundaries(ctx):
    """Runs over 31 | 32, exactly word 1, [31, 64], three whole words between partial neighbours, over the 64-word step at 2047 | 2048, two equal
    longest runs, the longest run ending at F - 1 with F % 32 != 0, and two rows of one atom pair with different timelines."""
    got = check(ctx, "run_boundaries")
    assert got["longest_run"].max() == tc.BOUNDARY_F


@pytest.mark.parametrize("kind", ["gap", "dense"])
def test_pass_sizes(ctx, kind):
    """The same schedule in passes of 5, 31, 32 and 33 frames and in one pass (the pass counts are asserted by check_reach): identical bytes.  gap:
    rows only in the first pass, only in the last partial pass, in both with a pass without pairs between; dense: runs across every pass boundary,
    two passes sharing a word."""
    name = f"passes_{kind}"
    tc.check_reach(name)
    c = tc.cases()[name]
    want = tc.expected_of(name)
    seen = set()
    for per in tc.PASS_SIZES:
        got = run(ctx, c.with_per(per))
        tc.assert_same(got, want)
        seen.add(to_bytes(got))
    assert len(seen) == 1


@pytest.mark.parametrize("R,order,pads", tc.ROW_COUNTS)
def test_row_counts(ctx, R, order, pads):
    """1, 2, 63, 64, 65, 128, 129 rows: both ends of the row search, one wave per row at the edges of k_timeline_stats' blocks of four; rows
    (2p + 1, 2p) and lone atoms in front."""
    got = check(ctx, f"rows_{R}")
    assert len(got["n_frames"]) == R


def test_mark_kernel_shapes(ctx):
    """A pair list of pairs with 1 and 2 set bits and a partly filled tail wave; coincident atoms (code 0)."""
    got = check(ctx, "mark_mixed")
    assert (got["interaction"] == 0).any()


def test_capacity(ctx):
    """timeline_cap_bytes one byte below rows x W x 4 is ARP_ERR_CAPACITY with rows, frames and bytes in the message; at exactly the need the table."""
    name = "passes_dense"
    c, want = tc.cases()[name], tc.expected_of(name)
    need = len(want["n_frames"]) * c.W * 4
    aa.debug_set("timeline_cap_bytes", need - 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        run(ctx, c)
    assert e.value.status == _lib.ARP_ERR_CAPACITY
    for part in (f"{len(want['n_frames'])} rows", f"{c.F} frames", f"{need} bytes"):
        assert part in str(e.value), str(e.value)
    aa.debug_set("timeline_cap_bytes", need)
    tc.assert_same(run(ctx, c), want)


@pytest.mark.parametrize("name", ["run_boundaries", "passes_gap"])
def test_no_bitmap(ctx, name):
    """ARP_TIMELINE_NO_BITMAP: the same statistics, no timeline_words, arp_table_timeline returns NULL."""
    c, want = tc.cases()[name], tc.expected_of(name)
    got = run(ctx, c, bitmap=False)
    assert "timeline_words" not in got and "n_total_frames" not in got
    tc.assert_same(got, want, bitmap=False)
    s = aa.Structure.from_records(c.top.rec)
    for bitmap in (False, True):
        t = aa.api._timeline_table(ctx, s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF, False, "atom", bitmap)
        try:
            wpr, nf = C.c_uint64(0), C.c_uint64(0)
            p = lib.arp_table_timeline(t, C.byref(wpr), C.byref(nf))
            assert (p is not None) == bitmap and (wpr.value, nf.value) == ((c.W, c.F) if bitmap else (0, 0))
        finally:
            lib.arp_table_free(t)


def test_other_tables_have_no_timeline(ctx):
    c = tc.cases()["passes_gap"]
    s = aa.Structure.from_records(c.top.rec)
    t = aa.api._freq_table(ctx, s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF)
    try:
        assert lib.arp_table_timeline(t, None, None) is None
        assert lib.arp_table_column(t, b"first_frame", None) is None
    finally:
        lib.arp_table_free(t)


def test_no_rows(ctx):
    top = fe.topology(["CC", "ON"], "AB")
    got = ctx.contact_timelines(aa.Structure.from_records(top.rec), fe.frames(top, fe.apart(40, 2)), "/", fe.VDW_COMP, fe.CUTOFF)
    assert got["timeline_words"].shape == (0, 2) and got["n_total_frames"] == 40 and all(len(got[c]) == 0 for c in tc.STAT_COLUMNS + fe.COLUMNS)


# ---- by definition on natural inputs -------------------------------------------------------------------------------------------------------------
def topology_xyz(s: aa.Structure, n: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)


def jittered(s: aa.Structure, n_frames: int, seed: int, sigma: float = 0.3) -> np.ndarray:
    n = aa.api._topology_atoms(s)
    return topology_xyz(s, n)[None] + np.random.default_rng(seed).normal(scale=sigma, size=(n_frames, n, 3))


def masks_of(key: np.ndarray, frame: np.ndarray, F: int) -> tuple:
    """Items (row key, frame) -> (sorted distinct keys, bool [R, F])."""
    uk, inv = np.unique(key, return_inverse=True)
    masks = np.zeros((len(uk), F), bool)
    masks[inv, frame] = True
    return uk, masks


def atom_key(i, j, code) -> np.ndarray:
    return (np.asarray(i).astype(np.uint64) << np.uint64(34)) | (np.asarray(j).astype(np.uint64) << np.uint64(5)) | np.asarray(code).astype(np.uint64)


def assert_timeline(got: dict, got_key: np.ndarray, uk: np.ndarray, masks: np.ndarray):
    """The rows are the expected rows in key order; bitmap, popcount and the five columns are those of the masks."""
    F = masks.shape[1]
    assert np.array_equal(got_key, uk)
    want = tc.stat_columns(masks)
    assert got["n_total_frames"] == F and np.array_equal(got["timeline_words"], want["timeline_words"])
    assert np.array_equal(aa.unpack_timeline(got["timeline_words"], F).sum(1), got["n_frames"])  # popcount == n_frames
    for c in tc.STAT_COLUMNS:
        assert got[c].dtype == want[c].dtype and np.array_equal(got[c].view(np.uint32), want[c].view(np.uint32)), c
    host = aa.timeline_stats(got["timeline_words"], F)
    assert np.array_equal(host["n_present"], got["n_frames"]) and np.array_equal(host["n_events"], got["n_events"])


def assert_frequency_parity(tl: dict, fq: dict):
    """Every column of the frequency call, byte for byte."""
    assert set(fq) <= set(tl) and set(tl) - set(fq) == set(tc.STAT_COLUMNS) | {"timeline_words", "n_total_frames"}
    for c in fq:
        assert tl[c].dtype == fq[c].dtype and tl[c].tobytes() == fq[c].tobytes(), c


@pytest.fixture(scope="module")
def natural(ctx, ubq_path, bft_path):
    """(structure, frames, groups, per-frame atom items) of the two natural inputs, computed once."""
    out = {}
    for which, path, F, groups in (("ubq", ubq_path, 70, "/"), ("bft", bft_path, 16, "H,L/C")):
        s = aa.load_model(path)
        frames = jittered(s, F, seed=F + len(groups))
        out[which] = (s, frames, groups, fc.atom_items(ctx, s, frames, groups))
    return out


@pytest.mark.parametrize("which,per", [("ubq", 25), ("bft", 5)])
def test_atom_level_by_definition(ctx, natural, which, per):
    s, frames, groups, (i, j, code, frame, _) = natural[which]
    F = frames.shape[0]
    uk, masks = masks_of(atom_key(i, j, code), frame, F)
    got = ctx.contact_timelines(s, frames, groups)
    assert_timeline(got, atom_key(got["from_atom"], got["to_atom"], got["interaction"]), uk, masks)
    assert (got["n_events"] > 1).any() and (got["longest_run"] == F).any()
    assert_frequency_parity(got, ctx.contact_frequencies(s, frames, groups))
    assert to_bytes(ctx.contact_timelines(s, frames, groups)) == to_bytes(got)  # repeatable
    assert F % per and -(-F // per) >= 3
    aa.debug_set("freq_chunk_atoms", per * frames.shape[1])
    assert to_bytes(ctx.contact_timelines(s, frames, groups)) == to_bytes(got)


@pytest.mark.parametrize("which,per", [("ubq", 25), ("bft", 5)])
def test_residue_level_by_definition(ctx, natural, which, per):
    """The same items grouped by (residue, residue, code, frame): residues with several atoms in contact in one frame set one bit."""
    s, frames, groups, (i, j, code, frame, _) = natural[which]
    F, n = frames.shape[0], frames.shape[1]
    res, _ = fc.topology_residues(s, n)
    uk, masks = masks_of(atom_key(res[i], res[j], code), frame, F)
    assert len(i) > masks.sum()  # more items than bits: several items of one frame set the same bit
    got = ctx.contact_timelines(s, frames, groups, level="residue")
    assert_timeline(got, atom_key(got["from_residue"], got["to_residue"], got["interaction"]), uk, masks)
    assert_frequency_parity(got, ctx.contact_frequencies(s, frames, groups, level="residue"))
    assert to_bytes(ctx.contact_timelines(s, frames, groups, level="residue")) == to_bytes(got)
    aa.debug_set("freq_chunk_atoms", per * n)
    aa.debug_set("freq_frame_bits", 2)
    assert to_bytes(ctx.contact_timelines(s, frames, groups, level="residue")) == to_bytes(got)


RING_F = 38


@pytest.fixture(scope="module")
def ring_input(ctx):
    """A ring topology of freq_ring_cases with 38 frames (ring-ring, ring-cation and altloc motifs), its per-frame atom items and, per frame, the
    ring rows of Context.get_contacts on the single-model structure of the frame: (from entity, to entity, code, frame) with ring e as n + e."""
    case = rg.build("timeline", ["rr"] * 3 + ["rc"] * 2 + ["alt"] + ["rr"] + ["rc"], F=RING_F, pads=20)
    s = aa.Structure.from_records(case.rec)
    n = case.frames.shape[1]
    ents = fcm.ring_entities(case.rec)
    items = []
    for f in range(RING_F):
        sf = aa.Structure.from_records(dict(case.rec, x=case.frames[f, :, 0].copy(), y=case.frames[f, :, 1].copy(), z=case.frames[f, :, 2].copy()))
        t = ctx.get_contacts(sf, "/", 0.1, 6.5)
        for k in np.flatnonzero((t["from_atom"] < 0) | (t["to_atom"] < 0)):
            e1 = ents[(bytes(t["from_chain"][k]), int(t["from_resi"][k]), bytes(t["from_insertion"][k]), bytes(t["from_altloc"][k]))]
            to = int(t["to_atom"][k]) if t["to_atom"][k] >= 0 else n + ents[(bytes(t["to_chain"][k]), int(t["to_resi"][k]), bytes(t["to_insertion"][k]), bytes(t["to_altloc"][k]))]
            items.append((n + e1, to, int(t["interaction"][k]), f))
    ring = np.array(items, np.int64).reshape(-1, 4)
    return case, s, fc.atom_items(ctx, s, case.frames, "/"), ring, fc.ring_items(ctx, s, case.rec, case.frames, "/")


@pytest.mark.parametrize("per", [None, 7])
def test_rings_atom_level(ctx, ring_input, per):
    case, s, (i, j, code, frame, _), ring, _ = ring_input
    n = case.frames.shape[1]
    assert (ring[:, 1] < n).any() and (ring[:, 1] >= n).any()  # ring - atom (CationPi) and ring - ring (Pi*) rows
    uk, masks = masks_of(np.concatenate([atom_key(i, j, code), atom_key(ring[:, 0], ring[:, 1], ring[:, 2])]), np.concatenate([frame, ring[:, 3]]), RING_F)
    if per:
        aa.debug_set("freq_chunk_atoms", per * n)
    got = ctx.contact_timelines(s, case.frames, "/", rings=True)
    ent = lambda atom, r: np.where(atom >= 0, atom, n + r)
    assert_timeline(got, atom_key(ent(got["from_atom"], got["from_ring"]), ent(got["to_atom"], got["to_ring"]), got["interaction"]), uk, masks)
    is_ring = got["from_ring"] >= 0
    assert is_ring.any() and is_ring[int(np.argmax(is_ring)):].all()  # ring rows follow atom rows
    assert (got["n_events"][is_ring] > 1).any()
    aa.debug_set("freq_chunk_atoms", 0)
    assert_frequency_parity(got, ctx.contact_frequencies(s, case.frames, "/", rings=True))
    # without rings: the atom rows, byte for byte
    plain = ctx.contact_timelines(s, case.frames, "/")
    for c in plain:
        if c != "n_total_frames":
            assert np.array_equal(plain[c], got[c][~is_ring]), c


@pytest.mark.parametrize("per,bits", [(None, 0), (7, 0), (None, 2)])
def test_rings_residue_level(ctx, ring_input, per, bits):
    case, s, (i, j, code, frame, _), _, (rA, rB, rcode, rframe, _) = ring_input
    n = case.frames.shape[1]
    res, _ = fc.topology_residues(s, n)
    assert len(rA) > 0
    uk, masks = masks_of(np.concatenate([atom_key(res[i], res[j], code), atom_key(rA, rB, rcode)]), np.concatenate([frame, rframe]), RING_F)
    aa.debug_set("freq_chunk_atoms", per * n if per else 0)
    aa.debug_set("freq_frame_bits", bits)
    got = ctx.contact_timelines(s, case.frames, "/", rings=True, level="residue")
    assert_timeline(got, atom_key(got["from_residue"], got["to_residue"], got["interaction"]), uk, masks)
    assert np.isin(got["interaction"], list(fc.RING_CODES)).any()
    aa.debug_set("freq_chunk_atoms", 0)
    aa.debug_set("freq_frame_bits", 0)
    assert_frequency_parity(got, ctx.contact_frequencies(s, case.frames, "/", rings=True, level="residue"))


def test_tiny_ring_buffers_grow(ctx, ring_input):
    """More ring items in a pass than the mark sweep's first item buffer holds (freq_cap_items sizes it): grown and repeated, the same bytes."""
    case, s = ring_input[0], ring_input[1]
    want = ctx.contact_timelines(s, case.frames, "/", rings=True)
    assert int(rg.items_per_frame(case).sum()) > 8
    aa.debug_set("freq_cap_items", 8)
    assert to_bytes(ctx.contact_timelines(s, case.frames, "/", rings=True)) == to_bytes(want)
    assert to_bytes(ctx.contact_timelines(s, case.frames, "/", rings=True, level="residue")) == to_bytes(
        (aa.debug_set("freq_cap_items", 0), ctx.contact_timelines(s, case.frames, "/", rings=True, level="residue"))[1])


def test_model_file(ctx, tmp_path, ubq_path):
    """A MODEL-record file with frames=None: the models are the frames; contact_timelines(path) and the command line give the same table."""
    from arpeggia_amd.__main__ import main

    rec = synth.read_pdb_records(ubq_path)
    F = 6
    rng = np.random.default_rng(8)
    parts = []
    for m in range(F):
        r = {k: v.copy() for k, v in rec.items()}
        for ax in ("x", "y", "z"):
            r[ax] = np.round(r[ax] + rng.normal(scale=0.3, size=len(r[ax])), 3)
        r["model_serial"][:] = m + 1
        parts.append(r)
    path = tmp_path / "ubq_models.pdb"
    synth.write_pdb({k: np.concatenate([p[k] for p in parts]) for k in rec}, path)
    s = aa.load_model(str(path))
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    frames = np.stack([soa["x"], soa["y"], soa["z"]], 1).reshape(F, n, 3)
    from_models = ctx.contact_timelines(s, None, "/")
    assert to_bytes(from_models) == to_bytes(ctx.contact_timelines(s, frames, "/"))
    i, j, code, frame, _ = fc.atom_items(ctx, s, frames, "/")
    uk, masks = masks_of(atom_key(i, j, code), frame, F)
    assert_timeline(from_models, atom_key(from_models["from_atom"], from_models["to_atom"], from_models["interaction"]), uk, masks)
    assert to_bytes(aa.contact_timelines(str(path))) == to_bytes(from_models)
    assert to_bytes(aa.get_contact_timelines(s, None, "/", bitmap=False)) == to_bytes({k: v for k, v in from_models.items() if k not in ("timeline_words", "n_total_frames")})
    # the command line: the frequency columns and the five timeline columns, in that order, and the bitmap file
    import pyarrow.parquet as pq

    assert main(["contact-timeline", "-i", str(path), "-o", str(tmp_path), "-t", "parquet", "--bitmap", str(tmp_path / "bits.npy")]) == 0
    table = pq.read_table(str(tmp_path / "contact_timeline.parquet"))
    assert table.column_names == [c for c, _ in aa.FREQ_COLUMNS] + tc.STAT_COLUMNS
    for c in tc.STAT_COLUMNS + ["n_frames", "from_atomi"]:
        assert np.array_equal(table.column(c).to_numpy(), from_models[c]), c
    assert np.array_equal(np.load(tmp_path / "bits.npy"), from_models["timeline_words"])
    freq = aa.get_contact_frequencies(s, None, "/")
    freq = freq if hasattr(freq, "column_names") else freq.to_arrow()
    for c in freq.column_names:
        assert table.column(c).to_pylist() == freq.column(c).to_pylist(), c
