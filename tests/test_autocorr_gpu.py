"""Contact autocorrelation and survival curves across frames (arp_contact_autocorrelation, arp_bit_autocorr) on the device.

arp_bit_autocorr puts k_acf_intermittent / k_acf_runs / k_acf_continuous on bitmaps at every lane, wave, tile, chunk and word edge (tests/autocorr_cases.py)
and compares the bytes with arp_bit_autocorr_host and with numpy.  End to end, the closed-form schedules of tests/timeline_cases.py are compared with numpy
on the schedule's masks, natural inputs with numpy on the bitmap of contact_timelines (a call with tests of its own) and, column by column, with the
frequency call.  Expected values never come from the autocorrelation call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import arpeggia_amd as aa
import autocorr_cases as ac
import freq_edge_cases as fe
import freq_ring_cases as rg
import similarity_cases as sc
import synth
import timeline_cases as tc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib

pytestmark = pytest.mark.gpu

KNOBS = ("freq_chunk_atoms", "freq_cap_items", "freq_frame_bits", "timeline_cap_bytes", "autocorr_cap_bytes")
EXTRA = {"half_life", "lags", "by_interaction", "mode", "n_total_frames"}


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


# ---- arp_bit_autocorr: the kernels on bitmaps ---------------------------------------------------------------------------------------------------
def check_bitmap(masks: np.ndarray, L: int, what="", words: np.ndarray | None = None, group=None, n_groups: int = 0, modes=ac.MODES) -> dict:
    """Device == host == numpy: the matrix, the half-lives and the sums, both modes, with and without the matrix."""
    masks = np.asarray(masks, bool)
    F = masks.shape[1]
    words = tc.pack(masks) if words is None else words
    out = {}
    for mode in modes:
        want = ac.reference(masks, L, mode, group, n_groups)
        got = aa.bit_autocorrelation(words, F, L, mode, group, n_groups, device=0)
        ac.assert_same(got, want, (what, mode))
        host = aa.bit_autocorrelation(words, F, L, mode, group, n_groups)
        assert all(got[k].tobytes() == host[k].tobytes() for k in host), (what, mode, "host")
        bare = aa.bit_autocorrelation(words, F, L, mode, group, n_groups, device=0, matrix=False)
        ac.assert_same(bare, want, (what, mode, "no matrix"), matrix=False)
        out[mode] = got
    return out


@pytest.mark.parametrize("L", ac.GPU_LAGS)
def test_lag_edges(ctx, L):
    """Lags at the lane (31 | 32), wave (63 | 64, 128 | 129) and tile (255 | 256) edges, on F = L + 1 and F = L + 34."""
    ac.check_bitmap_reach()
    for slack in ac.GPU_LAG_SLACK:
        F = L + slack
        check_bitmap(ac.pattern("random0.5", 3, F, seed=L * 3 + slack), L, (L, F))
        check_bitmap(ac.pattern("random0.99", 2, F, seed=L * 5 + slack), L, (L, F, "dense"))


@pytest.mark.parametrize("F", ac.GPU_FRAMES)
def test_frame_and_chunk_edges(ctx, F):
    """Frames at the bit and word edges, one staging chunk less a word / exact / a word more, two chunks and a word: two rows.  L = 70: the shifted
    operand lies two words and some bits ahead and crosses into the next chunk; L = 255: the tile's last lag reads the last word of the shifted window."""
    for L in sorted({min(F - 1, ac.CHUNK_L), min(F - 1, 3), min(F - 1, ac.LAGS_PER_BLOCK - 1)}):
        check_bitmap(ac.pattern("random0.5", 2, F, seed=F), L, (F, L))
    m = ac.pattern("random0.99", 2, F, seed=F + 1)  # long runs over the chunk edges
    check_bitmap(m, min(F - 1, ac.CHUNK_L), (F, "dense"))


def test_full_lag_range_over_several_tiles_and_chunks(ctx):
    """L = F - 1 with F beyond one staging chunk: every tile's chunk loop ends at its own triangle edge."""
    F = 32 * ac.CHUNK_WORDS + 77
    check_bitmap(ac.pattern("random0.9", 1, F, seed=4), F - 1, "full")


@pytest.mark.parametrize("R", ac.GPU_ROWS)
def test_row_edges(ctx, R):
    for F, L in ((40, 39), (97, 64)):
        check_bitmap(ac.pattern("random0.5", R, F, seed=R + F), L, (R, F), group=ac.groups_of(R, R), n_groups=ac.N_GROUPS)


@pytest.mark.parametrize("kind", [k for k in ac.PATTERNS if not k.startswith("random")])
def test_patterns(ctx, kind):
    for R, F in ((1, 1), (2, 33), (3, 65), (2, 1025)):
        check_bitmap(ac.pattern(kind, R, F), F - 1, (kind, R, F))


def test_run_staircase(ctx):
    """Row k is a single run of length k at a word-straddling offset: continuous counts are max(0, k - t)."""
    st = ac.staircase(70, 140)
    got = check_bitmap(st, 69, "staircase")
    assert np.array_equal(got["continuous"]["autocorrelation"], np.maximum(0, np.arange(70)[:, None] - np.arange(70)[None, :]))
    many = np.tile(ac.pattern("alternating", 1, 2 * ac.RUN_CHUNK * 2 + 40), (2, 1))  # more runs than one staged chunk of lengths
    many[1, 100:400] = True
    check_bitmap(many, 300, "many runs")


def test_touching_runs(ctx):
    """Two runs that reach a word boundary from each side without joining, and runs that cross it."""
    check_bitmap(ac.touching_runs(), 99, "touching")
    # the run lister's 64-word step: runs over bit 2048 | 2049, up to it and from it, and one over two whole steps and more
    edge = 32 * ac.RUN_STEP
    m = np.zeros((4, 2 * edge + 100), bool)
    m[0, edge - 20:edge + 30] = True
    m[1, edge - 20:edge] = True; m[1, edge + 1:edge + 9] = True
    m[2, 5:2 * edge + 50] = True
    m[3, edge:edge + 1] = True; m[3, edge - 2:edge - 1] = True
    check_bitmap(m, 120, "step edge")


def test_half_life_edges(ctx):
    """The integer predicate exactly on equality and one count to either side; a half-life beyond lane 63 of the row's first wave."""
    ac.check_bitmap_reach()
    m, F, t = ac.half_life_on_equality()
    got = check_bitmap(m, F - 1, "equality")
    assert got["intermittent"]["half_life"][0] == t and got["intermittent"]["half_life"][2] == t and got["intermittent"]["half_life"][1] != t
    late = ac.late_half_life()
    got = check_bitmap(late, late.shape[1] - 1, "late")
    assert got["intermittent"]["half_life"][0] == 93 and got["continuous"]["half_life"][0] == 93
    short = check_bitmap(late, 92, "one lag short")
    assert short["intermittent"]["half_life"][0] == ac.NONE


def test_dirty_bits_past_the_end(ctx):
    for R, F in ((1, 1), (5, 40), (33, 65), (2, 32 * ac.CHUNK_WORDS - 13)):
        m = sc.pattern("random0.5", R, F, seed=R + F)
        words = sc.dirty(tc.pack(m), F)
        assert not np.array_equal(words, tc.pack(m))
        check_bitmap(m, min(F - 1, 100), ("dirty", R, F), words=words)


def test_groups(ctx):
    """All rows in one group (the sum is contended), and 19 groups of which some stay empty."""
    m = ac.pattern("random0.5", 300, 200, seed=12)
    got = check_bitmap(m, 199, "one group", group=np.full(300, 5, "<u4"), n_groups=7)
    assert got["intermittent"]["sums"][5].tolist() == got["intermittent"]["autocorrelation"].astype(np.uint64).sum(0).tolist()
    got = check_bitmap(m, 199, "19 groups", group=ac.groups_of(300), n_groups=ac.N_GROUPS)
    assert not got["continuous"]["sums"][[3, 7, 18]].any()


def test_bitmap_capacity(ctx):
    m = ac.pattern("random0.5", 10, 40)
    aa.debug_set("autocorr_cap_bytes", 10 * 40 * 4 - 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        aa.bit_autocorrelation(tc.pack(m), 40, device=0)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "10 rows x 40 lags" in str(e.value) and "1600 bytes" in str(e.value)
    bare = aa.bit_autocorrelation(tc.pack(m), 40, device=0, matrix=False)  # without the matrix the limit does not apply
    ac.assert_same(bare, ac.reference(m, 39, "intermittent"), matrix=False)
    aa.debug_set("autocorr_cap_bytes", 10 * 40 * 4)
    check_bitmap(m, 39)


# ---- end to end: closed-form schedules -------------------------------------------------------------------------------------------------------------
def run(ctx, c: tc.Case, **kw) -> dict:
    s = aa.Structure.from_records(c.top.rec)
    assert s.n_atoms == c.top.n
    aa.debug_set("freq_chunk_atoms", c.chunk_atoms)
    return ctx.contact_autocorrelation(s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF, **kw)


def to_bytes(t: dict) -> bytes:
    parts = []
    for c in sorted(t):
        v = t[c]
        if isinstance(v, dict):
            parts.append(b"".join(k.encode() + v[k]["counts"].tobytes() + v[k]["curve"].tobytes() for k in sorted(v)))
        else:
            parts.append(np.ascontiguousarray(v).tobytes() if not isinstance(v, (str, int)) else str(v).encode())
    return b"".join(parts)


def assert_result(got: dict, masks: np.ndarray, codes, mode: str, L: int | None = None, what="", matrix: bool = True):
    """The matrix, the half-lives (f32, NaN: none), the lags and the per-interaction counts and curves against numpy on the masks."""
    R, F = masks.shape
    L = F - 1 if L is None else L
    want = ac.reference(masks, L, mode, codes, ac.N_INTERACTIONS)
    assert got["mode"] == mode and got["n_total_frames"] == F and np.array_equal(got["lags"], np.arange(L + 1))
    if matrix:
        a = got["autocorrelation"]
        assert a.dtype == np.dtype("<u4") and a.shape == (R, L + 1) and a.tobytes() == want["autocorrelation"].tobytes(), what
        assert np.array_equal(a[:, 0], got["n_frames"])
    else:
        assert "autocorrelation" not in got
    h = got["half_life"]
    assert h.dtype == np.dtype("<f4") and h.shape == (R,)
    none = want["half_life"] == ac.NONE
    assert np.array_equal(np.isnan(h), none) and np.array_equal(h[~none], want["half_life"][~none].astype(np.float32)), what
    present = [g for g in range(ac.N_INTERACTIONS) if want["sums"][g, 0]]
    assert list(got["by_interaction"]) == [_lib.INTERACTIONS[g] for g in present], what
    lags = np.arange(L + 1, dtype=np.float64)
    for g in present:
        entry = got["by_interaction"][_lib.INTERACTIONS[g]]
        assert entry["counts"].dtype == np.dtype("<u8") and entry["counts"].tobytes() == want["sums"][g].tobytes(), (what, g)
        curve = want["sums"][g].astype(np.float64) * F / (want["sums"][g][0].astype(np.float64) * (F - lags))
        assert entry["curve"].dtype == np.float64 and entry["curve"].tobytes() == curve.tobytes() and entry["curve"][0] == 1.0


@pytest.mark.parametrize("name", ac.CLOSED)
def test_closed_form(ctx, name):
    """The curves of a schedule equal numpy on the schedule's masks, both modes; the frequency columns are the closed form's.  F = 1, 33, 2049; 65 and 129
    rows; frames without any contact (passes_gap); runs over word and 64-word edges and an always-present row (run_boundaries)."""
    ac.check_reach(name)
    c, masks, codes, want = tc.cases()[name], ac.masks_of(name), ac.codes_of(name), tc.expected_of(name)
    for mode in ac.MODES:
        got = run(ctx, c, mode=mode)
        assert_result(got, masks, codes, mode, what=name)
        assert set(got) == set(fe.COLUMNS) | EXTRA | {"autocorrelation"}
        fe.assert_same_table({k: got[k] for k in fe.COLUMNS}, {k: want[k] for k in fe.COLUMNS})
    L = min(c.F - 1, 5)
    assert_result(run(ctx, c, mode="continuous", max_lag=L), masks, codes, "continuous", L, (name, "max_lag"))


@pytest.mark.parametrize("name", ac.CLOSED)
def test_closed_form_residue_level(ctx, name):
    """Every atom of these topologies is a residue of its own, so the residue-level rows are the atom-level rows in some order: the curves are numpy on the
    residue-level bitmap of contact_timelines, whose rows are the schedule's masks.  All seven schedules, both modes."""
    ac.check_reach(name)
    c = tc.cases()[name]
    s = aa.Structure.from_records(c.top.rec)
    tl = ctx.contact_timelines(s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF, level="residue")
    res_masks = aa.unpack_timeline(tl["timeline_words"], c.F)
    assert sorted(map(bytes, res_masks)) == sorted(map(bytes, ac.masks_of(name)))
    for mode in ac.MODES:
        got = run(ctx, c, level="residue", mode=mode)
        assert_result(got, res_masks, tl["interaction"].astype("<u4"), mode, what=name)
        assert got["from_residue"].tobytes() == tl["from_residue"].tobytes()


@pytest.mark.parametrize("level", ["atom", "residue"])
def test_no_contact_in_any_frame(ctx, level):
    """R = 0: a 0 x (L + 1) matrix, zero sums (no interaction has rows), no half-life."""
    top, D = sc.no_contact_case(40)
    s = aa.Structure.from_records(top.rec)
    for mode in ac.MODES:
        got = ctx.contact_autocorrelation(s, fe.frames(top, D), "/", fe.VDW_COMP, fe.CUTOFF, level=level, mode=mode, max_lag=7)
        assert got["autocorrelation"].shape == (0, 8) and got["autocorrelation"].dtype == np.dtype("<u4")
        assert got["by_interaction"] == {} and got["half_life"].shape == (0,) and len(got["n_frames"]) == 0 and got["n_total_frames"] == 40
    t = aa.api._autocorr_table(ctx, s, fe.frames(top, D), "/", fe.VDW_COMP, fe.CUTOFF, False, level, "intermittent", 7, True)
    try:
        n_lags, n_groups, sums = C.c_uint64(), C.c_uint32(), C.POINTER(C.c_uint64)()
        assert lib.arp_table_autocorrelation(t, C.byref(n_lags), None, C.byref(sums), C.byref(n_groups)) is not None
        assert n_lags.value == 8 and n_groups.value == ac.N_INTERACTIONS and not any(sums[k] for k in range(8 * ac.N_INTERACTIONS))
    finally:
        lib.arp_table_free(t)


@pytest.mark.parametrize("kind", ["gap", "dense"])
def test_pass_sizes(ctx, kind):
    """The same schedule in passes of 5, 31, 32 and 33 frames and in one pass (gap: with passes without any pair): identical bytes."""
    name = f"passes_{kind}"
    tc.check_reach(name)
    c, masks, codes = tc.cases()[name], ac.masks_of(name), ac.codes_of(name)
    for mode in ac.MODES:
        seen = set()
        for per in tc.PASS_SIZES:
            got = run(ctx, c.with_per(per), mode=mode)
            assert_result(got, masks, codes, mode, what=(name, per))
            seen.add(to_bytes(got))
        assert len(seen) == 1


def test_capacity(ctx):
    """autocorr_cap_bytes one byte below R x (L + 1) x 4 is ARP_ERR_CAPACITY with rows, lags and bytes in the message; at exactly the need the matrix.  The
    need is known only after the rows sweep; without the matrix the limit does not apply; the bitmap's own limit still does."""
    name = "passes_dense"
    c, masks, codes = tc.cases()[name], ac.masks_of(name), ac.codes_of(name)
    R = masks.shape[0]
    for L in (c.F - 1, 9):
        need = R * (L + 1) * 4
        aa.debug_set("autocorr_cap_bytes", need - 1)
        with pytest.raises(aa.ArpeggiaError) as e:
            run(ctx, c, max_lag=L)
        assert e.value.status == _lib.ARP_ERR_CAPACITY
        for part in (f"{R} rows x {L + 1} lags", f"{need} bytes", "autocorr_cap_bytes"):
            assert part in str(e.value), str(e.value)
        assert_result(run(ctx, c, max_lag=L, matrix=False), masks, codes, "intermittent", L, matrix=False)
        aa.debug_set("autocorr_cap_bytes", need)
        assert_result(run(ctx, c, max_lag=L), masks, codes, "intermittent", L)
    aa.debug_set("autocorr_cap_bytes", 0)
    aa.debug_set("timeline_cap_bytes", R * c.W * 4 - 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        run(ctx, c, matrix=False)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "timeline_cap_bytes" in str(e.value)


def test_no_matrix(ctx):
    """ARP_ACF_NO_MATRIX: no matrix, the same half-lives and sums; arp_table_autocorrelation returns NULL and still hands out the sums."""
    name = "run_boundaries"
    c, masks, codes = tc.cases()[name], ac.masks_of(name), ac.codes_of(name)
    for mode in ac.MODES:
        full, bare = run(ctx, c, mode=mode), run(ctx, c, mode=mode, matrix=False)
        assert_result(bare, masks, codes, mode, what=name, matrix=False)
        full.pop("autocorrelation")
        assert to_bytes(full) == to_bytes(bare)
    s = aa.Structure.from_records(c.top.rec)
    xyz = fe.frames(c.top, c.D)
    t = aa.api._autocorr_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF, False, "atom", "continuous", None, False)
    try:
        n_lags, flags, n_groups, sums = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.POINTER(C.c_uint64)()
        assert lib.arp_table_autocorrelation(t, C.byref(n_lags), C.byref(flags), C.byref(sums), C.byref(n_groups)) is None
        assert n_lags.value == c.F and flags.value == _lib.ARP_ACF_CONTINUOUS | _lib.ARP_ACF_NO_MATRIX and n_groups.value == ac.N_INTERACTIONS and bool(sums)
        assert lib.arp_table_timeline(t, None, None) is None and lib.arp_table_similarity(t, None, None, None) is None
        assert lib.arp_table_column(t, b"half_life", None) is not None and lib.arp_table_column(t, b"first_frame", None) is None
    finally:
        lib.arp_table_free(t)
    for other in (aa.api._freq_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF), aa.api._timeline_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF, False, "atom", True)):
        try:
            assert lib.arp_table_autocorrelation(other, None, None, None, None) is None and lib.arp_table_column(other, b"half_life", None) is None
        finally:
            lib.arp_table_free(other)


# ---- end to end: natural inputs -----------------------------------------------------------------------------------------------------------------------
def jittered(s: aa.Structure, n_frames: int, seed: int, sigma: float = 0.3) -> np.ndarray:
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    xyz = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
    return xyz[None] + np.random.default_rng(seed).normal(scale=sigma, size=(n_frames, n, 3))


def assert_frequency_parity(got: dict, fq: dict):
    """Every column of the frequency call, byte for byte, and nothing else but the autocorrelation's own keys."""
    assert set(fq) <= set(got) and set(got) - set(fq) == EXTRA | {"autocorrelation"}
    for c in fq:
        assert got[c].dtype == fq[c].dtype and got[c].tobytes() == fq[c].tobytes(), c


def check_natural(ctx, s, frames, groups, per: int, rings: bool = False):
    """Both levels, both modes: numpy on the bitmap of contact_timelines; the frequency columns; repeatable; the same bytes in forced passes."""
    F, n = frames.shape[0], frames.shape[1]
    for level in ("atom", "residue"):
        tl = ctx.contact_timelines(s, frames, groups, rings=rings, level=level)
        masks = aa.unpack_timeline(tl["timeline_words"], F)
        fq = ctx.contact_frequencies(s, frames, groups, rings=rings, level=level)
        codes = tl["interaction"].astype("<u4")
        for mode in ac.MODES:
            got = ctx.contact_autocorrelation(s, frames, groups, rings=rings, level=level, mode=mode)
            assert_result(got, masks, codes, mode, what=(level, mode))
            assert_frequency_parity(got, fq)
        assert to_bytes(ctx.contact_autocorrelation(s, frames, groups, rings=rings, level=level, mode=mode)) == to_bytes(got)  # repeatable
        assert F % per and -(-F // per) >= 3
        aa.debug_set("freq_chunk_atoms", per * n)
        assert to_bytes(ctx.contact_autocorrelation(s, frames, groups, rings=rings, level=level, mode=mode)) == to_bytes(got)
        aa.debug_set("freq_chunk_atoms", 0)
    return masks


def test_ubq_70_frames(ctx, ubq_path):
    s = aa.load_model(ubq_path)
    masks = check_natural(ctx, s, jittered(s, 70, seed=71), "/", per=25)
    assert masks.shape[0] > ac.ROWS_PER_BLOCK  # (the residue-level rows: more than one block of the run lister)


def test_bft_16_frames_chain_groups(ctx, bft_path):
    s = aa.load_model(bft_path)
    check_natural(ctx, s, jittered(s, 16, seed=21), "H,L/C", per=5)


def test_ring_topology(ctx):
    """A ring topology of freq_ring_cases, rings on: the ring rows have curves and feed the sums of their interactions."""
    case = rg.build("autocorrelation", ["rr"] * 3 + ["rc"] * 2 + ["alt"] + ["rr"] + ["rc"], F=38, pads=20)
    s = aa.Structure.from_records(case.rec)
    for level in ("atom", "residue"):
        tl = ctx.contact_timelines(s, case.frames, "/", rings=True, level=level)
        masks = aa.unpack_timeline(tl["timeline_words"], 38)
        fq = ctx.contact_frequencies(s, case.frames, "/", rings=True, level=level)
        for mode in ac.MODES:
            got = ctx.contact_autocorrelation(s, case.frames, "/", rings=True, level=level, mode=mode)
            assert_result(got, masks, tl["interaction"].astype("<u4"), mode, what=(level, mode))
            assert_frequency_parity(got, fq)
        aa.debug_set("freq_chunk_atoms", 7 * case.frames.shape[1])
        assert to_bytes(ctx.contact_autocorrelation(s, case.frames, "/", rings=True, level=level, mode=mode)) == to_bytes(got)
        aa.debug_set("freq_chunk_atoms", 0)
        plain = ctx.contact_autocorrelation(s, case.frames, "/", level=level)
        assert len(plain["n_frames"]) < len(got["n_frames"]) and set(plain["by_interaction"]) < set(got["by_interaction"])


def test_over_the_cap_is_refused_before_the_marks(ctx, ubq_path):
    """A call whose R x (L + 1) x 4 exceeds the (lowered) limit is refused as soon as R is known, and the context goes on working."""
    s = aa.load_model(ubq_path)
    frames = jittered(s, 8, seed=3)
    R = len(ctx.contact_frequencies(s, frames, "/", level="residue")["n_frames"])
    aa.debug_set("autocorr_cap_bytes", R * 4)
    with pytest.raises(aa.ArpeggiaError) as e:
        ctx.contact_autocorrelation(s, frames, "/", level="residue")
    assert e.value.status == _lib.ARP_ERR_CAPACITY and f"{R} rows x 8 lags" in str(e.value) and f"{R * 8 * 4} bytes" in str(e.value)
    got = ctx.contact_autocorrelation(s, frames, "/", level="residue", max_lag=0)  # R x 1 fits
    assert got["autocorrelation"].shape == (R, 1) and np.isnan(got["half_life"]).all()


def test_model_file(ctx, tmp_path, ubq_path):
    """A MODEL-record file with frames=None: the models are the frames; contact_autocorrelation(path) and the command line give the same counts, the
    frequency call's table with half_life behind it, and the curves."""
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
    from_models = ctx.contact_autocorrelation(s, None, "/")
    assert from_models["n_total_frames"] == F and to_bytes(from_models) == to_bytes(ctx.contact_autocorrelation(s, frames, "/"))
    tl = ctx.contact_timelines(s, None, "/")
    assert_result(from_models, aa.unpack_timeline(tl["timeline_words"], F), tl["interaction"].astype("<u4"), "intermittent")
    assert to_bytes(aa.contact_autocorrelation(str(path))) == to_bytes(from_models)
    assert to_bytes(aa.get_contact_autocorrelation(s, None, "/", mode="continuous", max_lag=3)) == to_bytes(ctx.contact_autocorrelation(s, frames, "/", mode="continuous", max_lag=3))
    import pyarrow.parquet as pq

    assert main(["contact-autocorrelation", "-i", str(path), "-o", str(tmp_path), "-t", "parquet", "--matrix", str(tmp_path / "acf.npy"), "--curves", str(tmp_path / "c.csv")]) == 0
    table = pq.read_table(str(tmp_path / "contact_autocorrelation.parquet"))
    assert table.column_names == [c for c, _ in aa.FREQ_COLUMNS] + ["half_life"]
    freq = aa.get_contact_frequencies(s, None, "/")
    freq = freq if hasattr(freq, "column_names") else freq.to_arrow()
    for c in freq.column_names:
        assert table.column(c).to_pylist() == freq.column(c).to_pylist(), c
    want_hl = [None if np.isnan(v) else float(v) for v in from_models["half_life"]]
    assert table.column("half_life").to_pylist() == want_hl
    saved = np.load(tmp_path / "acf.npy")
    assert saved.dtype == np.uint32 and saved.tobytes() == from_models["autocorrelation"].tobytes()
    lines = (tmp_path / "c.csv").read_text().splitlines()
    names = list(from_models["by_interaction"])
    assert lines[0] == ",".join(["lag"] + names) and len(lines) == F + 1
    for k, line in enumerate(lines[1:]):
        cells = line.split(",")
        assert int(cells[0]) == k and [float(v) for v in cells[1:]] == [float(from_models["by_interaction"][n]["curve"][k]) for n in names]
    assert main(["contact-autocorrelation", "-i", str(path), "-o", str(tmp_path), "-l", "residue", "--mode", "continuous", "--max-lag", "2", "--matrix", str(tmp_path / "r.npy")]) == 0
    want = ctx.contact_autocorrelation(s, None, "/", level="residue", mode="continuous", max_lag=2)
    assert np.load(tmp_path / "r.npy").tobytes() == want["autocorrelation"].tobytes()
