"""Residue-level contact frequencies across frames (arp_residue_contact_frequencies; level="residue") on the device.

Built cases (tests/freq_residue_cases.py: fat residues on the 1/256 A grid) are compared with their closed form, every column for equality, after
the layout prediction has shown that the case still reaches the edge it is named for; tests/test_freq_residue_host.py pins the closed form to the
oracle on the CPU.  Natural inputs are compared with the table by definition: one Context.atomic_contacts call per frame (and, with rings, one
Context.get_contacts call per frame) grouped by residue in numpy -- tests/freq_residue_common.py.  Expected values never come from the residue
call itself.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import freq_residue_cases as rr
import freq_residue_common as fc
import freq_ring_cases as rg
import synth
from freq_common import ring_entities

pytestmark = pytest.mark.gpu

KNOBS = ("freq_chunk_atoms", "freq_cap_items", "freq_frame_bits")


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


def knobs(chunk_atoms: int = 0, cap: int = 0, bits: int = 0):
    for k, v in zip(KNOBS, (chunk_atoms, cap, bits)):
        aa.debug_set(k, v)


def run(ctx, name: str, unforced: bool = False) -> dict:
    """The case on the device with its own knobs (unforced: with none), after the case's reach assertions."""
    rr.check_reach(name)
    c = rr.cases()[name]
    s = aa.Structure.from_records(c.top.rec)
    assert s.n_atoms == c.top.n
    if unforced:
        knobs()
    else:
        knobs(c.chunk_atoms, c.cap, c.frame_bits)
    return ctx.contact_frequencies(s, c.frames(), "/", rr.ec.VDW_COMP, rr.ec.CUTOFF, level="residue")


@pytest.mark.parametrize("name", list(rr.cases()))
def test_built_cases(ctx, name):
    """semantics: dedup, union, closest approach, codes kept apart.  subruns*: (row, frame) sub-runs of 64 and 65 items, across sorted position
    255 -> 256, single items at lanes 63 and 0, a row over more than three waves, with and without the aggregate's entry in front.  passes*: the
    same residue pair in the last frame of one pass and the first of the next, aggregate-only, new and carried rows in one pass, passes without
    pairs in front and in the middle, buffers of one item, two frame bits.  many_frames: two passes under the cap of 65 535 frames.  one_frame,
    no_contact: the trivial tables."""
    got = run(ctx, name)
    rr.assert_same_table(got, rr.reference_of(name))
    c = rr.cases()[name]
    if c.chunk_atoms or c.cap or c.frame_bits:
        assert fc.to_bytes(run(ctx, name, unforced=True)) == fc.to_bytes(got)
    if name == "no_contact":
        assert set(got) == set(rr.COLUMNS) and all(len(v) == 0 for v in got.values())


def test_union_against_the_atom_table(ctx):
    """Pair 0 on even frames, pair 1 on odd frames: the atom table says 0.5 and 0.5, the residue row says 1.0; and the closest-approach group has
    an atom row with max_distance 4.25 where the residue row has 3.5."""
    c = rr.cases()["semantics"]
    s = aa.Structure.from_records(c.top.rec)
    atom = ctx.contact_frequencies(s, c.frames(), "/")
    res_t = ctx.contact_frequencies(s, c.frames(), "/", level="residue")
    res, _ = rr.residues(c.top.rec)
    A, B = rr.pair_of(c, 1)
    sel = (res[atom["from_atom"]] == A) & (res[atom["to_atom"]] == B) & (atom["interaction"] == 18)
    assert atom["frequency"][sel].tolist() == [0.5, 0.5]
    k = (res_t["from_residue"] == A) & (res_t["to_residue"] == B) & (res_t["interaction"] == 18)
    assert res_t["frequency"][k].tolist() == [1.0] and res_t["n_frames"][k].tolist() == [c.F]
    A, B = rr.pair_of(c, 2)
    sel = (res[atom["from_atom"]] == A) & (res[atom["to_atom"]] == B) & (atom["interaction"] == 18)
    k = (res_t["from_residue"] == A) & (res_t["to_residue"] == B) & (res_t["interaction"] == 18)
    assert atom["max_distance"][sel].max() == np.float32(4.25) and res_t["max_distance"][k].tolist() == [3.5]
    fc.assert_consistent_with_atom_table(res_t, atom, res, c.F)


@pytest.mark.parametrize("name", ["semantics", "subruns_second_pass", "passes"])
@pytest.mark.parametrize("how", ["frame_bits_2", "frame_bits_1", "three_passes", "four_passes", "both"])
def test_pass_size_and_frame_cap_do_not_change_the_bytes(ctx, name, how):
    c = rr.cases()[name]
    want = rr.reference_of(name)
    s = aa.Structure.from_records(c.top.rec)
    bits = {"frame_bits_2": 2, "frame_bits_1": 1, "both": 2}.get(how, 0)
    passes = {"three_passes": 3, "four_passes": 4, "both": 4}.get(how, 0)
    chunk = -(-c.F // passes) * c.top.n if passes else 0
    per = rr.frames_per_pass(c, chunk_atoms=chunk, knob=bits)
    lay = rr.layout(c, per=per, cap0=0)
    if bits:  # at most 2^bits - 1 frames per pass: the cap binds unless the pass size asks for fewer still
        by_size = -(-c.F // passes) if passes else c.F
        assert per == min((1 << bits) - 1, by_size) and (how != "both" or name == "semantics" or per < by_size)
        assert len(lay) == -(-c.F // per) and max(r.key[1] for ps in lay for r in ps.sub) == per
    else:
        assert len(lay) == passes and per == -(-c.F // passes)
    knobs(chunk, 0, bits)
    got = ctx.contact_frequencies(s, c.frames(), "/", rr.ec.VDW_COMP, rr.ec.CUTOFF, level="residue")
    rr.assert_same_table(got, want)
    knobs()
    assert fc.to_bytes(ctx.contact_frequencies(s, c.frames(), "/", rr.ec.VDW_COMP, rr.ec.CUTOFF, level="residue")) == fc.to_bytes(got)


# ---- rings -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_rings(ctx):
    case = rg.small_case()
    s = aa.Structure.from_records(case.rec)
    return case, s, fc.expected(ctx, s, case.frames, "/", rec=case.rec), fc.expected(ctx, s, case.frames, "/")


@pytest.mark.parametrize("mode", ["one_pass", "three_passes", "frame_bits_2", "tiny_buffers"])
def test_ring_rows_by_residue(ctx, small_rings, mode):
    """freq_ring_cases' small case: an "alt" motif's two ring entities are one residue row, "rc" rows run from the ring's residue to the LYS, and
    the ring rows of an "rr" pair stand beside the atom rows of the same residue pair under their own codes."""
    case, s, want, want_atoms = small_rings
    K = len(case.kinds)
    if mode == "three_passes":
        assert "partial" in rg.edges(case, case.per_for_passes(3))
        knobs(case.per_for_passes(3) * case.n)
    elif mode == "frame_bits_2":
        knobs(bits=2)
    elif mode == "tiny_buffers":
        assert int(rg.items_per_frame(case).sum()) > 48
        knobs(cap=48)
    got = ctx.contact_frequencies(s, case.frames, "/", rings=True, level="residue")
    fc.assert_same_table(got, want)
    ring = np.isin(got["interaction"], list(fc.RING_CODES))
    closed = rr.ring_reference(case)
    for col in ("from_residue", "to_residue", "interaction", "n_frames", "frequency"):
        assert np.array_equal(got[col][ring], closed[col].astype(got[col].dtype)), col
    assert np.abs(got["min_distance"][ring] - closed["min_distance"]).max() <= 1e-5 and np.abs(got["max_distance"][ring] - closed["max_distance"]).max() <= 1e-5
    # alt: one row per code where the atom-level table has two (one per ring entity)
    p = case.kinds.index("alt")
    atom_level = ctx.contact_frequencies(s, case.frames, "/", rings=True)
    n_alt_entity_rows = int(np.isin(atom_level["from_ring"], case.a_ring[p]).sum())
    n_alt_residue_rows = int((ring & (got["from_residue"] == p)).sum())
    assert n_alt_entity_rows == 2 * n_alt_residue_rows > 0
    # rc: CationPi from the ring's residue to the cation's
    q = case.kinds.index("rc")
    cp = ring & (got["interaction"] == 17) & (got["from_residue"] == q)
    assert cp.sum() == 1 and got["to_residue"][cp][0] == K + case.pads + q and got["from_resn"][cp][0] == b"PHE" and got["to_resn"][cp][0] == b"LYS"
    # rr: atom rows and ring rows of one residue pair, each under its own codes
    r = case.kinds.index("rr")
    pair = (got["from_residue"] == r) & (got["to_residue"] == K + case.pads + r)
    assert (pair & ring).any() and (pair & ~ring).any()
    # without the flag: the atom items alone
    knobs()
    fc.assert_same_table(ctx.contact_frequencies(s, case.frames, "/", level="residue"), want_atoms)
    res, _ = rr.residues(case.rec)
    ents = ring_entities(case.rec)
    of = {(bytes(case.rec["chain"][k]), int(case.rec["resi"][k]), bytes(case.rec["icode"][k])): int(res[k]) for k in range(case.n)}
    ring_res = np.array([of[key[:3]] for key in ents], np.int64)
    fc.assert_consistent_with_atom_table(got, atom_level, res, case.F, ring_res)


# ---- natural inputs --------------------------------------------------------------------------------------------------------------------------
def topology_xyz(s: aa.Structure) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)


def jittered(s: aa.Structure, F: int, seed: int, sigma: float = 0.3) -> np.ndarray:
    base = topology_xyz(s)
    return base[None] + np.random.default_rng(seed).normal(scale=sigma, size=(F,) + base.shape)


NATURAL = [("ubq", 64, "/"), ("bft", 16, "/"), ("bft", 16, "H,L/C"), ("bft", 16, "C/H"), ("stress", 32, "/")]


@pytest.fixture(scope="module")
def inputs(ubq_path, bft_path):
    stress = synth.gen_stress(n_res=150, seed=11)
    recs = {"ubq": synth.read_pdb_records(ubq_path), "bft": synth.read_pdb_records(bft_path), "stress": stress}
    structs = {"ubq": aa.load_model(ubq_path), "bft": aa.load_model(bft_path), "stress": aa.Structure.from_records(stress)}
    frames = {(name, F): jittered(structs[name], F, seed=100 + F) for name, F, _ in NATURAL}
    return recs, structs, frames


@pytest.fixture(scope="module")
def references(ctx, inputs):
    """(input, groups) -> (atom items, ring items), one device loop each, shared by every test below."""
    recs, structs, frames = inputs
    out = {}
    for name, F, groups in NATURAL:
        s, fr = structs[name], frames[(name, F)]
        res, _ = fc.topology_residues(s, fr.shape[1])
        i, j, code, frame, dist = fc.atom_items(ctx, s, fr, groups)
        out[(name, groups)] = ((res[i], res[j], code, frame, dist), fc.ring_items(ctx, s, recs[name], fr, groups))
    return out


@pytest.mark.parametrize("name,F,groups", NATURAL)
@pytest.mark.parametrize("rings", [False, True])
@pytest.mark.parametrize("forced", [False, True])
def test_natural_inputs(ctx, inputs, references, name, F, groups, rings, forced):
    recs, structs, frames = inputs
    s, fr = structs[name], frames[(name, F)]
    n = fr.shape[1]
    atoms, ring = references[(name, groups)]
    items = tuple(np.concatenate(v) for v in zip(atoms, ring)) if rings else atoms
    want = fc.group_by_residue(s, F, n, *items)
    assert len(want["n_frames"]) > 0 and ((want["frequency"] > 0) & (want["frequency"] < 1)).any()
    if rings and name != "ubq" and groups == "/":  # (1ubq has rings, none in contact: tests/test_freq_rings_gpu.py)
        assert len(ring[0]) > 0
    if forced:  # three passes by size, and inside them the frame cap of two bits
        knobs(chunk_atoms=-(-F // 3) * n, bits=2)
    got = ctx.contact_frequencies(s, fr, groups, rings=rings, level="residue")
    fc.assert_same_table(got, want)
    again = ctx.contact_frequencies(s, fr, groups, rings=rings, level="residue")
    assert fc.to_bytes(again) == fc.to_bytes(got)  # two calls, identical bytes
    if not forced:
        # the fat rows are there: some row has more items than frames (the atom table cannot give its count)
        res, _ = fc.topology_residues(s, n)
        atom_t = ctx.contact_frequencies(s, fr, groups, rings=rings)
        ring_res = None
        if rings:
            chain, resi, ins = s.strings("chain")[:n], s.ints("resi")[:n], s.strings("insertion")[:n]
            of = {(bytes(chain[k]), int(resi[k]), bytes(ins[k])): int(res[k]) for k in range(n)}
            ring_res = np.array([of[key[:3]] for key in ring_entities(recs[name])], np.int64)
        fc.assert_consistent_with_atom_table(got, atom_t, res, F, ring_res)
        assert len(atom_t["n_frames"]) > len(got["n_frames"])


@pytest.mark.parametrize("name", ["ubq", "bft"])
def test_one_frame_is_the_group_by_of_the_atom_table(ctx, inputs, name):
    recs, structs, frames = inputs
    s = structs[name]
    fr = topology_xyz(s)[None]
    n = fr.shape[1]
    res, _ = fc.topology_residues(s, n)
    atom_t = ctx.contact_frequencies(s, fr, "/")
    got = ctx.contact_frequencies(s, fr, "/", level="residue")
    fc.assert_consistent_with_atom_table(got, atom_t, res, 1)
    want = fc.group_by_residue(s, 1, n, res[atom_t["from_atom"]], res[atom_t["to_atom"]], atom_t["interaction"].astype(np.int64), np.zeros(len(atom_t["interaction"]), np.int64),
                               atom_t["min_distance"])
    fc.assert_same_table(got, want)
    from_models = ctx.contact_frequencies(s, None, "/", level="residue")
    assert fc.to_bytes(from_models) == fc.to_bytes(got)


def test_arrow_table_and_column_set(ctx, inputs):
    recs, structs, frames = inputs
    s, fr = structs["ubq"], frames[("ubq", 64)]
    cols = ctx.contact_frequencies(s, fr, "/", level="residue")
    table = aa.get_contact_frequencies(s, fr, "/", level="residue")
    if hasattr(table, "to_arrow"):  # a polars.DataFrame when polars is there
        table = table.to_arrow()
    assert table.column_names == [c for c, _ in aa.RESIDUE_FREQ_COLUMNS] and table.num_rows == len(cols["n_frames"])
    get = lambda c: np.array(table.column(c).to_pylist())
    for c in ("n_frames", "frequency", "min_distance", "max_distance", "from_resi", "to_resi"):
        assert np.array_equal(get(c), cols[c]), c
    assert [str(v) for v in get("from_chain")] == [v.decode() for v in cols["from_chain"]]
    assert [str(v) for v in get("interaction")] == [aa._lib.INTERACTIONS[k] for k in cols["interaction"]]
    # the atom-level keyword path is untouched
    assert fc.to_bytes(ctx.contact_frequencies(s, fr, "/", level="atom")) == fc.to_bytes(ctx.contact_frequencies(s, fr, "/"))
    with pytest.raises(ValueError):
        ctx.contact_frequencies(s, fr, "/", level="chain")


def test_cli_end_to_end(ctx, tmp_path):
    """contact-frequency --level residue --rings on a MODEL-record file: the table of the Python call, which is the table by definition."""
    from arpeggia_amd.__main__ import main

    case = rg.small_case()
    F = 9
    fr = np.round(case.frames[:F], 3)
    parts = []
    for m in range(F):
        r = {k: v.copy() for k, v in rg.frame_records(case, m, fr).items()}
        r["model_serial"][:] = m + 1
        parts.append(r)
    path = tmp_path / "small_models.pdb"
    synth.write_pdb({k: np.concatenate([p[k] for p in parts]) for k in case.rec}, path)
    rec0 = rg.frame_records(case, 0, fr)
    want = fc.expected(ctx, aa.Structure.from_records(rec0), fr, "/", rec=rec0)
    got = ctx.contact_frequencies(aa.load_model(str(path)), None, "/", rings=True, level="residue")
    fc.assert_same_table(got, want)
    out = tmp_path / "out"
    assert main(["contact-frequency", "-i", str(path), "-o", str(out), "--rings", "-l", "residue"]) == 0
    import pyarrow.csv as pacsv

    csv = pacsv.read_csv(str(out / "contact_frequency.csv"))
    assert csv.column_names == [c for c, _ in aa.RESIDUE_FREQ_COLUMNS] and csv.num_rows == len(want["n_frames"]) > 0
    assert csv.column("n_frames").to_pylist() == want["n_frames"].tolist()
    assert csv.column("from_resi").to_pylist() == want["from_resi"].tolist() and csv.column("to_resi").to_pylist() == want["to_resi"].tolist()
    assert csv.column("interaction").to_pylist() == [aa._lib.INTERACTIONS[k] for k in want["interaction"]]
    assert np.allclose(np.array(csv.column("min_distance").to_pylist()), want["min_distance"], rtol=0, atol=1e-6)
    assert np.allclose(np.array(csv.column("max_distance").to_pylist()), want["max_distance"], rtol=0, atol=1e-6)
    assert "CationPi" in csv.column("interaction").to_pylist()
    plain = tmp_path / "plain"
    assert main(["contact-frequency", "-i", str(path), "-o", str(plain), "--rings"]) == 0
    assert pacsv.read_csv(str(plain / "contact_frequency.csv")).column_names == [c for c, _ in aa.FREQ_COLUMNS]
