"""Ring rows of contact frequencies across frames (arp_contact_frequencies_ex with ARP_FREQ_RINGS) on the device.

The reference for bytes is the device's own single-structure path: for every frame, the single-model structure of the topology's records with the
frame's coordinates (Structure.from_records), Context.get_contacts, the rows with a Ring entity, aggregated by entity pair and code in numpy.  Every
column of the ring rows must be equal, row order included; the atom rows must be the table without rings, byte for byte.  The built cases of
tests/freq_ring_cases.py are also held against their closed form.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import arpeggia_amd as aa
import freq_ring_cases as rc
import synth
from arpeggia_amd import _lib
from arpeggia_amd.api import _frames_arg, _np_from
from freq_common import BASE, RING_ATOMS, assert_same_rows, atom_part, device_reference, ring_entities, ring_part  # noqa: F401

pytestmark = pytest.mark.gpu

PI_CODES = set(range(11, 17))
CATION_PI = 17


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    aa.debug_set("freq_chunk_atoms", 0)
    aa.debug_set("freq_cap_items", 0)


def to_bytes(t: dict, cols=None) -> bytes:
    return b"".join(np.ascontiguousarray(t[c]).tobytes() for c in sorted(cols or t))


def check(ctx, s, rec, frames, groups, want=None, dist_cutoff=6.5):
    """rings=True against the reference and against rings=False; returns (table, reference)."""
    want = device_reference(ctx, rec, frames, groups, dist_cutoff) if want is None else want
    got = ctx.contact_frequencies(s, frames, groups, 0.1, dist_cutoff, rings=True)
    assert set(got) == set(BASE) | {"from_ring", "to_ring"}
    assert_same_rows(ring_part(got), want)
    plain = ctx.contact_frequencies(s, frames, groups, 0.1, dist_cutoff)
    assert set(plain) == set(BASE)
    assert to_bytes(atom_part(got)) == to_bytes(plain)
    return got, want


def topology_xyz(s: aa.Structure) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)


def jittered(s: aa.Structure, F: int, seed: int, sigma: float = 0.3) -> np.ndarray:
    base = topology_xyz(s)
    return base[None] + np.random.default_rng(seed).normal(scale=sigma, size=(F,) + base.shape)


@pytest.fixture(scope="module")
def bft(bft_path):
    return aa.load_model(bft_path), synth.read_pdb_records(bft_path)


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path), synth.read_pdb_records(ubq_path)


def test_bft_single_frame_is_the_golden_table(ctx, bft):
    s, rec = bft
    frames = topology_xyz(s)[None]
    got, _ = check(ctx, s, rec, frames, "/")
    from_file = ctx.contact_frequencies(s, None, "/", rings=True)
    assert to_bytes(from_file) == to_bytes(got)
    ring = ring_part(got)
    codes, counts = np.unique(ring["interaction"], return_counts=True)
    # tests/golden/6bft_contacts.csv: 24 PiTiltedStacking, 17 CationPi, 8 PiLStacking, 7 PiDisplacedStacking, 4 PiParallelInPlaneStacking
    assert dict(zip(codes.tolist(), counts.tolist())) == {15: 24, 17: 17, 16: 8, 11: 7, 14: 4}
    assert (ring["n_frames"] == 1).all() and (ring["frequency"] == 1.0).all() and np.array_equal(ring["min_distance"], ring["max_distance"])
    assert (ring["from_atomn"] == b"Ring").all() and (ring["from_atomi"] == 0).all() and (ring["from_atom"] == -1).all()


@pytest.fixture(scope="module")
def bft_jitter(ctx, bft):
    s, rec = bft
    frames = jittered(s, 8, seed=17)
    return frames, {g: device_reference(ctx, rec, frames, g) for g in ("/", "H,L/C")}


@pytest.mark.parametrize("groups", ["/", "H,L/C"])
@pytest.mark.parametrize("passes", [1, 3])
def test_bft_jittered_frames(ctx, bft, bft_jitter, groups, passes):
    s, rec = bft
    frames, refs = bft_jitter
    want = refs[groups]
    codes = set(want["interaction"].tolist())
    if groups == "/":  # the case must not go vacuous
        assert len(codes) >= 5 and CATION_PI in codes and codes <= PI_CODES | {CATION_PI}
    else:
        assert len(want["interaction"]) >= 1
    if passes == 3:
        per = 3  # 3 + 3 + 2 frames
        assert frames.shape[0] % per and -(-frames.shape[0] // per) == 3
        aa.debug_set("freq_chunk_atoms", per * frames.shape[1])
    got, _ = check(ctx, s, rec, frames, groups, want)
    f = ring_part(got)["frequency"]
    assert ((f > 0) & (f < 1)).any()


def test_ubq_rings_present_none_in_contact(ctx, ubq):
    s, rec = ubq
    assert len(ring_entities(rec)) > 0
    frames = jittered(s, 16, seed=16)
    got, want = check(ctx, s, rec, frames, "/")
    assert len(want["interaction"]) == 0 and (got["from_ring"] == -1).all() and len(got["from_ring"]) > 0


@pytest.fixture(scope="module")
def case_refs(ctx):
    return {c.name: device_reference(ctx, c.rec, c.frames, "/") for c in rc.all_cases()}


def assert_closed_form(ring: dict, want: dict):
    for c in ("interaction", "n_frames", "frequency", "from_ring", "to_ring", "from_atom", "to_atom", "from_resi", "to_resi"):
        assert np.array_equal(ring[c], want[c].astype(ring[c].dtype)), c
    for c in ("from_chain", "from_altloc", "to_chain", "to_atomn"):
        assert np.array_equal(ring[c], want[c].astype(ring[c].dtype)), c
    assert (ring["from_atomn"] == b"Ring").all() and (ring["from_resn"] == b"PHE").all() and (ring["from_atomi"] == 0).all()


@pytest.mark.parametrize("case", rc.all_cases(), ids=lambda c: c.name)
@pytest.mark.parametrize("mode", ["one_pass", "three_passes", "tiny_buffers"])
def test_built_cases(ctx, case_refs, case, mode):
    # the case reaches its wave / block / pass edges (asserted again here: the device run below is only worth something if it does)
    per = case.F if mode != "three_passes" else case.per_for_passes(3)
    reached = rc.edges(case, per)
    assert {"fit64", "fit128", "fit256", "items64"} <= reached
    assert "items256" in reached or mode == "three_passes"
    if mode == "three_passes":
        assert "partial" in reached
    if case.name == "small":
        assert "keybit" in reached
    if case.name == "wide":
        assert {"tile2", "ring64", "ring256", "cand64", "cand256"} <= reached
    s = aa.Structure.from_records(case.rec)
    unforced = ctx.contact_frequencies(s, case.frames, "/", rings=True)
    if mode == "three_passes":
        aa.debug_set("freq_chunk_atoms", per * case.n)
    if mode == "tiny_buffers":  # the first buffers hold fewer items than one pass's ring items: grown, expand and ring kernels repeated
        assert int(rc.items_per_frame(case).sum()) > 48
        aa.debug_set("freq_cap_items", 48)
    got, want = check(ctx, s, case.rec, case.frames, "/", case_refs[case.name])
    assert to_bytes(got) == to_bytes(unforced)
    assert_closed_form(ring_part(got), rc.expected(case))


def test_small_cutoff_keeps_the_ring_ring_rows(ctx):
    case = rc.small_case()
    assert rc.min_distance_between_residues(case) > 1.0
    s = aa.Structure.from_records(case.rec)
    got = ctx.contact_frequencies(s, case.frames, "/", 0.1, 1.0, rings=True)
    assert (got["from_ring"] >= 0).all() and (got["to_ring"] >= 0).all()  # no atom row in any frame, no CationPi row
    assert CATION_PI not in set(got["interaction"].tolist())
    assert_closed_form(got, rc.expected(case, ring_ring_only=True))
    assert len(ctx.contact_frequencies(s, case.frames, "/", 0.1, 1.0)["interaction"]) == 0
    nine = ctx.contact_frequencies(s, case.frames[:9], "/", 0.1, 1.0, rings=True)
    assert_same_rows(nine, device_reference(ctx, case.rec, case.frames[:9], "/", 1.0))


def test_topology_without_rings(ctx):
    import freq_edge_cases as ec

    top = ec.topology(["CC", "ON", "OO", "ON"])
    D = np.array([[3.0, 3.0, 2.75, 8.0], [4.0, 3.5, 3.5, 3.0], [8.0, 8.0, 8.0, 8.0]])
    frames = ec.frames(top, D)
    s = aa.Structure.from_records(top.rec)
    with_rings = ctx.contact_frequencies(s, frames, "/", rings=True)
    plain = ctx.contact_frequencies(s, frames, "/")
    assert len(plain["interaction"]) > 0
    assert to_bytes(with_rings, BASE) == to_bytes(plain)
    assert (with_rings["from_ring"] == -1).all() and (with_rings["to_ring"] == -1).all()
    table = aa.get_contact_frequencies(s, frames, "/", rings=True)
    assert len(table) == len(plain["interaction"])


def old_entry_point(ctx, s, frames, groups: str) -> dict:
    n_frames, ptr, keep = _frames_arg(s, frames, "contact frequencies")
    t = C.c_void_p()
    assert _lib.lib.arp_contact_frequencies(ctx._h, s._h, int(n_frames), ptr, groups.encode(), 0.1, 6.5, C.byref(t)) == _lib.ARP_OK
    try:
        n = int(_lib.lib.arp_table_rows(t))
        out = {}
        for name, kind in aa.FREQ_COLUMNS + [("from_atom", "i4"), ("to_atom", "i4")]:
            w = C.c_int32()
            p = _lib.lib.arp_table_column(t, name.encode(), C.byref(w))
            assert p
            out[name] = _np_from(p, n, "<i4" if name == "interaction" else (f"S{max(w.value, 1)}" if kind == "str" else "<" + kind))
        return out
    finally:
        _lib.lib.arp_table_free(t)


def test_no_flag_is_the_old_entry_point(ctx, bft):
    s, _ = bft
    frames = jittered(s, 4, seed=4)
    new = ctx.contact_frequencies(s, frames, "/")
    old = old_entry_point(ctx, s, frames, "/")
    assert len(old["interaction"]) > 0 and to_bytes(new) == to_bytes(old)


@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    """Nine frames of the small case as a MODEL-record file (coordinates rounded to the file's 3 decimals first)."""
    case = rc.small_case()
    F = 9
    frames = np.round(case.frames[:F], 3)
    parts = []
    for m in range(F):
        r = {k: v.copy() for k, v in rc.frame_records(case, m, frames).items()}
        r["model_serial"][:] = m + 1
        parts.append(r)
    path = tmp_path_factory.mktemp("freq_rings") / "small_models.pdb"
    synth.write_pdb({k: np.concatenate([p[k] for p in parts]) for k in case.rec}, path)
    return case, frames, str(path)


def test_model_file_equals_the_array_form(ctx, model_file):
    case, frames, path = model_file
    s = aa.load_model(path)
    assert s.n_atoms == frames.shape[0] * case.n
    from_models = ctx.contact_frequencies(s, None, "/", rings=True)
    from_arrays = ctx.contact_frequencies(s, topology_xyz(s).reshape(frames.shape), "/", rings=True)
    assert to_bytes(from_models) == to_bytes(from_arrays)
    # the rings are those of model 0 as a single-model structure: the table of that structure with the same frames
    single = aa.Structure.from_records(rc.frame_records(case, 0, frames))
    assert to_bytes(from_models) == to_bytes(ctx.contact_frequencies(single, frames, "/", rings=True))
    ring = ring_part(from_models)
    assert len(ring["interaction"]) > 0 and set(ring["from_altloc"].tolist()) == {b"", b"A", b"B"}
    assert_same_rows(ring, device_reference(ctx, rc.frame_records(case, 0, frames), frames, "/"))


def test_two_calls_give_identical_bytes(ctx, bft):
    s, _ = bft
    frames = jittered(s, 8, seed=17)
    a = ctx.contact_frequencies(s, frames, "/", rings=True)
    b = ctx.contact_frequencies(s, frames, "/", rings=True)
    assert to_bytes(a) == to_bytes(b) and (a["from_ring"] >= 0).any()
    ta, tb = aa.get_contact_frequencies(s, frames, "/", rings=True), aa.get_contact_frequencies(s, frames, "/", rings=True)
    assert ta.equals(tb) and len(ta) == len(a["interaction"])


def test_cli_rings_end_to_end(tmp_path, model_file):
    from arpeggia_amd.__main__ import main

    _, _, path = model_file
    out = tmp_path / "out"
    assert main(["contact-frequency", "-i", path, "-o", str(out), "--rings"]) == 0
    import pyarrow.csv as pacsv

    csv = pacsv.read_csv(str(out / "contact_frequency.csv"))
    want = aa.contact_frequencies(path, rings=True)
    plain = aa.contact_frequencies(path)
    assert csv.num_rows == len(want) > len(plain)
    assert csv.column_names == [c for c, _ in aa.FREQ_COLUMNS]
    assert csv.column("from_atomn").to_pylist().count("Ring") == len(want) - len(plain)
    assert "CationPi" in csv.column("interaction").to_pylist()
