"""Contact similarity between frames and contact co-occurrence between rows (arp_contact_similarity, arp_bit_gram) on the device.

arp_bit_gram puts k_bit_transpose / k_bit_sizes / k_bit_gram on bitmaps at every tile, chunk and word edge (tests/similarity_cases.py) and compares
the bytes with arp_bit_gram_host and with numpy.  End to end, the closed-form schedules of tests/timeline_cases.py are compared with numpy on the
schedule's masks, natural inputs with numpy on the bitmap of contact_timelines (a call with tests of its own) and, column by column, with the
frequency call.  Expected values never come from the similarity call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import arpeggia_amd as aa
import freq_edge_cases as fe
import freq_ring_cases as rg
import similarity_cases as sc
import synth
import timeline_cases as tc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib

pytestmark = pytest.mark.gpu

KNOBS = ("freq_chunk_atoms", "freq_cap_items", "freq_frame_bits", "timeline_cap_bytes", "similarity_cap_bytes")
EXTRA = {"sizes", "axis", "n_total_frames"}


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


def to_bytes(t: dict) -> bytes:
    return b"".join(np.ascontiguousarray(t[c]).tobytes() if not isinstance(t[c], (str, int)) else str(t[c]).encode() for c in sorted(t))


# ---- arp_bit_gram: the kernels on bitmaps -------------------------------------------------------------------------------------------------------
def check_bitmap(masks: np.ndarray, axes=sc.AXES, words: np.ndarray | None = None, what=""):
    """Device == host == numpy, matrix and sizes, both metrics."""
    masks = np.asarray(masks, bool)
    n_bits = masks.shape[1]
    words = tc.pack(masks) if words is None else words
    for axis in axes:
        want = sc.reference(masks, axis)
        for metric in sc.METRICS:
            got, sizes = aa.bit_gram(words, n_bits, axis, metric, device=0)
            sc.assert_matrix(got, sizes, masks, axis, metric, what, want)
            host, host_sizes = aa.bit_gram(words, n_bits, axis, metric)
            assert got.tobytes() == host.tobytes() and sizes.tobytes() == host_sizes.tobytes(), (what, axis, metric)


@pytest.mark.parametrize("M", sc.GRAM_M)
def test_gram_tile_and_chunk_edges(ctx, M):
    """k_bit_gram alone (axis "rows"): M around one, two and three tiles, K at 1 word, one chunk less a word, a chunk, a chunk and a word, two chunks and
    a word, each with a full and with a partial last word."""
    sc.check_bitmap_reach()
    for K in sc.GRAM_K:
        for n_bits in sc.gram_bits(K):
            check_bitmap(sc.pattern("random0.5", M, n_bits, seed=M * 131 + n_bits), ("rows",), what=(M, K, n_bits))


@pytest.mark.parametrize("R", sc.TRANSPOSE_R)
def test_transpose_edges(ctx, R):
    """Axis "frames" (k_bit_transpose in front): rows around one, two and three 32-row tiles, frames from one bit to 33 words."""
    for F in sc.TRANSPOSE_F:
        check_bitmap(sc.pattern("random0.5", R, F, seed=R * 977 + F), ("frames",), what=(R, F))


@pytest.mark.parametrize("kind", sc.EDGE_PATTERNS)
def test_patterns(ctx, kind):
    """All ones, all zeros (empty unions: 1.0), a checkerboard, a single set bit in the last valid position; both axes."""
    for R, F in sc.EDGE_SHAPES:
        check_bitmap(sc.pattern(kind, R, F), what=(kind, R, F))


def test_dirty_bits_past_the_end(ctx):
    """Set bits past n_bits in every row's last word change nothing."""
    for R, F in ((1, 1), (5, 40), (sc.TILE + 1, 32 * sc.CHUNK - sc.GRAM_TAIL), (33, 65), (100, 1025 - 32 + 7)):
        m = sc.pattern("random0.5", R, F, seed=R + F)
        words = sc.dirty(tc.pack(m), F)
        assert not np.array_equal(words, tc.pack(m))
        check_bitmap(m, words=words, what=("dirty", R, F))


def test_mirror_is_a_transpose(ctx):
    """Row k has its first k bits set: tiles (0, 1) and (1, 0) of the matrix differ, so a mirror written without transposing (or not at all) shows."""
    sc.check_bitmap_reach()
    R, F = sc.MIRROR_SHAPE
    m = sc.pattern("staircase", R, F)
    check_bitmap(m, what="staircase")
    got, _ = aa.bit_gram(tc.pack(m), F, "rows", "count", device=0)
    assert np.array_equal(got, got.T) and not np.array_equal(got[:sc.TILE, sc.TILE:2 * sc.TILE], got[sc.TILE:2 * sc.TILE, :sc.TILE])


def test_bitmap_capacity(ctx):
    m = sc.pattern("random0.5", 10, 40)
    aa.debug_set("similarity_cap_bytes", 40 * 40 * 4 - 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        aa.bit_gram(tc.pack(m), 40, "frames", "count", device=0)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "M = 40" in str(e.value) and "6400 bytes" in str(e.value) and "frames" in str(e.value)
    check_bitmap(m, ("rows",))  # 10 x 10 fits


# ---- end to end: closed-form schedules -------------------------------------------------------------------------------------------------------------
def run(ctx, c: tc.Case, **kw) -> dict:
    s = aa.Structure.from_records(c.top.rec)
    assert s.n_atoms == c.top.n
    aa.debug_set("freq_chunk_atoms", c.chunk_atoms)
    return ctx.contact_similarity(s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF, **kw)


def assert_result(got: dict, masks: np.ndarray, axis: str, metric: str, what="", want: dict | None = None):
    key = sc.KEY[metric]
    assert key in got and sc.KEY[{"tanimoto": "count", "count": "tanimoto"}[metric]] not in got
    assert got["axis"] == axis and got["n_total_frames"] == masks.shape[1]
    sc.assert_matrix(got[key], got["sizes"], masks, axis, metric, what, want)
    M = masks.shape[1] if axis == "frames" else masks.shape[0]
    assert got[key].shape == (M, M)
    if metric == "tanimoto" and M:
        assert (np.diag(got[key]) == 1.0).all()
    if axis == "rows":
        assert np.array_equal(got["sizes"], got["n_frames"])


@pytest.mark.parametrize("name", sc.CLOSED)
def test_closed_form(ctx, name):
    """The matrix of a schedule equals numpy on the schedule's masks: both axes, both metrics; the frequency columns are the closed form's.  F = 1, 33,
    2049; 1, 65, 129 rows; frames without any contact (passes_gap); K over two chunks with a partial last word (run_boundaries, axis "rows")."""
    sc.check_reach(name)
    c, masks, want = tc.cases()[name], sc.masks_of(name), tc.expected_of(name)
    for axis in sc.AXES:
        for metric in sc.METRICS:
            got = run(ctx, c, axis=axis, metric=metric)
            assert_result(got, masks, axis, metric, name)
            assert set(got) == set(fe.COLUMNS) | EXTRA | {sc.KEY[metric]}
            fe.assert_same_table({k: got[k] for k in fe.COLUMNS}, {k: want[k] for k in fe.COLUMNS})


@pytest.mark.parametrize("name", ["frames_33", "rows_65", "passes_gap"])
def test_closed_form_residue_level(ctx, name):
    """Every atom of these topologies is a residue of its own, so the residue-level rows are the atom-level rows in some order: between frames the
    matrix is that of the schedule's masks; between rows it is numpy on the residue-level bitmap of contact_timelines."""
    c, masks = tc.cases()[name], sc.masks_of(name)
    s = aa.Structure.from_records(c.top.rec)
    tl = ctx.contact_timelines(s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF, level="residue")
    res_masks = aa.unpack_timeline(tl["timeline_words"], c.F)
    assert sorted(map(bytes, res_masks)) == sorted(map(bytes, masks))
    for metric in sc.METRICS:
        assert_result(run(ctx, c, level="residue", metric=metric), masks, "frames", metric, name)
        got = run(ctx, c, level="residue", axis="rows", metric=metric)
        assert_result(got, res_masks, "rows", metric, name)
        assert got["from_residue"].tobytes() == tl["from_residue"].tobytes()


@pytest.mark.parametrize("level", ["atom", "residue"])
def test_no_contact_in_any_frame(ctx, level):
    """R = 0: between frames the counts are 0, the Tanimoto values 1.0 and the sizes 0; between rows the matrix is empty."""
    top, D = sc.no_contact_case(40)
    s = aa.Structure.from_records(top.rec)
    args = (s, fe.frames(top, D), "/", fe.VDW_COMP, fe.CUTOFF)
    got = ctx.contact_similarity(*args, level=level)
    assert got["similarity"].shape == (40, 40) and got["similarity"].dtype == np.dtype("<f4") and (got["similarity"] == 1.0).all()
    assert got["sizes"].shape == (40,) and not got["sizes"].any() and len(got["n_frames"]) == 0 and got["n_total_frames"] == 40
    got = ctx.contact_similarity(*args, level=level, metric="count")
    assert got["intersection"].shape == (40, 40) and got["intersection"].dtype == np.dtype("<u4") and not got["intersection"].any()
    for metric in sc.METRICS:
        got = ctx.contact_similarity(*args, level=level, axis="rows", metric=metric)
        assert got[sc.KEY[metric]].shape == (0, 0) and got["sizes"].shape == (0,) and got["axis"] == "rows"


@pytest.mark.parametrize("kind", ["gap", "dense"])
def test_pass_sizes(ctx, kind):
    """The same schedule in passes of 5, 31, 32 and 33 frames and in one pass (gap: with passes without any pair): identical bytes."""
    name = f"passes_{kind}"
    tc.check_reach(name)
    c, masks = tc.cases()[name], sc.masks_of(name)
    for axis in sc.AXES:
        seen = set()
        for per in tc.PASS_SIZES:
            got = run(ctx, c.with_per(per), axis=axis)
            assert_result(got, masks, axis, "tanimoto", (name, per))
            seen.add(to_bytes(got))
        assert len(seen) == 1


def test_capacity(ctx):
    """similarity_cap_bytes one byte below M x M x 4 is ARP_ERR_CAPACITY with M, the axis and the bytes in the message; at exactly the need the matrix.
    Between rows the need is known only after the rows sweep."""
    name = "passes_dense"
    c, masks = tc.cases()[name], sc.masks_of(name)
    for axis, M in (("frames", c.F), ("rows", masks.shape[0])):
        need = M * M * 4
        aa.debug_set("similarity_cap_bytes", need - 1)
        with pytest.raises(aa.ArpeggiaError) as e:
            run(ctx, c, axis=axis)
        assert e.value.status == _lib.ARP_ERR_CAPACITY
        for part in (f"M = {M}", f"axis {axis}", f"{need} bytes", "similarity_cap_bytes"):
            assert part in str(e.value), str(e.value)
        aa.debug_set("similarity_cap_bytes", need)
        assert_result(run(ctx, c, axis=axis), masks, axis, "tanimoto")
    aa.debug_set("similarity_cap_bytes", 0)
    aa.debug_set("timeline_cap_bytes", masks.shape[0] * c.W * 4 - 1)  # the bitmap's own limit still applies
    with pytest.raises(aa.ArpeggiaError) as e:
        run(ctx, c)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "timeline_cap_bytes" in str(e.value)


def test_table_handle(ctx):
    """arp_table_similarity serves the matrix of a similarity table and NULL for every other table; the similarity table has no timeline columns."""
    c = tc.cases()["passes_gap"]
    s = aa.Structure.from_records(c.top.rec)
    xyz = fe.frames(c.top, c.D)
    t = aa.api._similarity_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF, False, "atom", "rows", "count")
    try:
        m, flags, sizes = C.c_uint64(), C.c_uint32(), C.POINTER(C.c_uint32)()
        assert lib.arp_table_similarity(t, C.byref(m), C.byref(flags), C.byref(sizes)) is not None
        assert m.value == sc.masks_of("passes_gap").shape[0] and flags.value == _lib.ARP_SIM_ROWS | _lib.ARP_SIM_COUNTS and bool(sizes)
        assert lib.arp_table_similarity(t, None, None, None) is not None
        assert lib.arp_table_timeline(t, None, None) is None and lib.arp_table_column(t, b"first_frame", None) is None
    finally:
        lib.arp_table_free(t)
    for other in (aa.api._freq_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF), aa.api._timeline_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF, False, "atom", True)):
        try:
            assert lib.arp_table_similarity(other, None, None, None) is None
        finally:
            lib.arp_table_free(other)


# ---- end to end: natural inputs -----------------------------------------------------------------------------------------------------------------------
def jittered(s: aa.Structure, n_frames: int, seed: int, sigma: float = 0.3) -> np.ndarray:
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    xyz = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
    return xyz[None] + np.random.default_rng(seed).normal(scale=sigma, size=(n_frames, n, 3))


def assert_frequency_parity(sim: dict, fq: dict, metric: str):
    """Every column of the frequency call, byte for byte, and nothing else but the matrix, sizes, axis and n_total_frames."""
    assert set(fq) <= set(sim) and set(sim) - set(fq) == EXTRA | {sc.KEY[metric]}
    for c in fq:
        assert sim[c].dtype == fq[c].dtype and sim[c].tobytes() == fq[c].tobytes(), c


def check_natural(ctx, s, frames, groups, per: int, rings: bool = False):
    """Between frames at both levels and between rows at residue level: numpy on the bitmap of contact_timelines; the frequency columns; repeatable;
    the same bytes in forced passes."""
    F, n = frames.shape[0], frames.shape[1]
    for level, axes in (("atom", ("frames",)), ("residue", sc.AXES)):
        tl = ctx.contact_timelines(s, frames, groups, rings=rings, level=level)
        masks = aa.unpack_timeline(tl["timeline_words"], F)
        fq = ctx.contact_frequencies(s, frames, groups, rings=rings, level=level)
        assert masks.any(0).all()
        for axis in axes:
            want = sc.reference(masks, axis)
            for metric in sc.METRICS:
                got = ctx.contact_similarity(s, frames, groups, rings=rings, level=level, axis=axis, metric=metric)
                assert_result(got, masks, axis, metric, (level, axis, metric), want)
                assert_frequency_parity(got, fq, metric)
            assert to_bytes(ctx.contact_similarity(s, frames, groups, rings=rings, level=level, axis=axis, metric=metric)) == to_bytes(got)  # repeatable
            assert F % per and -(-F // per) >= 3
            aa.debug_set("freq_chunk_atoms", per * n)
            assert to_bytes(ctx.contact_similarity(s, frames, groups, rings=rings, level=level, axis=axis, metric=metric)) == to_bytes(got)
            aa.debug_set("freq_chunk_atoms", 0)
    return masks


def test_ubq_70_frames(ctx, ubq_path):
    s = aa.load_model(ubq_path)
    masks = check_natural(ctx, s, jittered(s, 70, seed=71), "/", per=25)
    assert masks.shape[0] > 3 * sc.TILE  # (the residue-level rows: more than three tiles between rows)
    sim = sc.reference(masks, "frames")["similarity"]
    assert 0.0 < sim.min() < sim.max() == 1.0 and (sim[~np.eye(70, dtype=bool)] < 1.0).all()  # jittered frames: alike, never identical


def test_bft_16_frames_chain_groups(ctx, bft_path):
    s = aa.load_model(bft_path)
    check_natural(ctx, s, jittered(s, 16, seed=21), "H,L/C", per=5)


def test_ring_topology(ctx):
    """A ring topology of freq_ring_cases, rings on: the ring rows take part in both matrices; without rings the frames' sizes are smaller."""
    case = rg.build("similarity", ["rr"] * 3 + ["rc"] * 2 + ["alt"] + ["rr"] + ["rc"], F=38, pads=20)
    s = aa.Structure.from_records(case.rec)
    for level in ("atom", "residue"):
        tl = ctx.contact_timelines(s, case.frames, "/", rings=True, level=level)
        masks = aa.unpack_timeline(tl["timeline_words"], 38)
        fq = ctx.contact_frequencies(s, case.frames, "/", rings=True, level=level)
        for axis in sc.AXES:
            for metric in sc.METRICS:
                got = ctx.contact_similarity(s, case.frames, "/", rings=True, level=level, axis=axis, metric=metric)
                assert_result(got, masks, axis, metric, (level, axis, metric))
                assert_frequency_parity(got, fq, metric)
        aa.debug_set("freq_chunk_atoms", 7 * case.frames.shape[1])
        assert to_bytes(ctx.contact_similarity(s, case.frames, "/", rings=True, level=level, axis=axis, metric=metric)) == to_bytes(got)
        aa.debug_set("freq_chunk_atoms", 0)
        plain = ctx.contact_similarity(s, case.frames, "/", level=level, metric="count")
        with_rings = ctx.contact_similarity(s, case.frames, "/", rings=True, level=level, metric="count")
        assert (plain["sizes"] <= with_rings["sizes"]).all() and (plain["sizes"] < with_rings["sizes"]).any()


def test_rows_axis_over_the_cap_is_refused(ctx, ubq_path):
    """Between rows the matrix grows with the square of the table: a call whose R x R x 4 exceeds the (lowered) limit is refused before the marks sweep,
    and the context goes on working."""
    s = aa.load_model(ubq_path)
    frames = jittered(s, 8, seed=3)
    R = len(ctx.contact_frequencies(s, frames, "/", level="residue")["n_frames"])
    aa.debug_set("similarity_cap_bytes", 1 << 16)
    assert R * R * 4 > 1 << 16
    with pytest.raises(aa.ArpeggiaError) as e:
        ctx.contact_similarity(s, frames, "/", level="residue", axis="rows")
    assert e.value.status == _lib.ARP_ERR_CAPACITY and f"M = {R}" in str(e.value) and f"{R * R * 4} bytes" in str(e.value) and "axis rows" in str(e.value)
    got = ctx.contact_similarity(s, frames, "/", level="residue")  # 8 x 8 fits
    assert got["similarity"].shape == (8, 8)


def test_model_file(ctx, tmp_path, ubq_path):
    """A MODEL-record file with frames=None: the models are the frames; contact_similarity(path) and the command line give the same matrix and the
    frequency call's table."""
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
    from_models = ctx.contact_similarity(s, None, "/")
    assert from_models["n_total_frames"] == F and to_bytes(from_models) == to_bytes(ctx.contact_similarity(s, frames, "/"))
    masks = aa.unpack_timeline(ctx.contact_timelines(s, None, "/")["timeline_words"], F)
    assert_result(from_models, masks, "frames", "tanimoto")
    assert to_bytes(aa.contact_similarity(str(path))) == to_bytes(from_models)
    assert to_bytes(aa.get_contact_similarity(s, None, "/", metric="count")) == to_bytes(ctx.contact_similarity(s, frames, "/", metric="count"))
    import pyarrow.parquet as pq

    assert main(["contact-similarity", "-i", str(path), "-o", str(tmp_path), "-t", "parquet", "--matrix", str(tmp_path / "sim.npy")]) == 0
    table = pq.read_table(str(tmp_path / "contact_similarity.parquet"))
    assert table.column_names == [c for c, _ in aa.FREQ_COLUMNS]
    freq = aa.get_contact_frequencies(s, None, "/")
    freq = freq if hasattr(freq, "column_names") else freq.to_arrow()
    for c in freq.column_names:
        assert table.column(c).to_pylist() == freq.column(c).to_pylist(), c
    saved = np.load(tmp_path / "sim.npy")
    assert saved.dtype == np.float32 and saved.tobytes() == from_models["similarity"].tobytes()
    assert main(["contact-similarity", "-i", str(path), "-o", str(tmp_path), "-l", "residue", "--axis", "rows", "--metric", "count", "--matrix", str(tmp_path / "co.npy")]) == 0
    want = ctx.contact_similarity(s, None, "/", level="residue", axis="rows", metric="count")
    assert np.load(tmp_path / "co.npy").tobytes() == want["intersection"].tobytes()
