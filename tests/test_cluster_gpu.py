"""Clusters of the frames by their contacts (arp_contact_clusters, arp_bit_cluster) on the device.

arp_bit_cluster puts k_bit_transpose / k_bit_sizes / k_bit_adjacency / k_cluster_round / k_cluster_tail / k_cluster_counts on bitmaps at every word and tile
edge and on the directed cases of tests/cluster_cases.py, and compares the bytes of every output with arp_bit_cluster_host and with numpy.  End to end, the
closed-form schedules of tests/timeline_cases.py are compared with numpy on the schedule's masks, natural inputs with numpy on the matrix of contact_similarity
and the bitmap of contact_timelines (calls with tests of their own) and, column by column, with the frequency call.  Expected values never come from the
cluster call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import arpeggia_amd as aa
import cluster_cases as cc
import freq_edge_cases as fe
import freq_ring_cases as rg
import similarity_cases as sc
import synth
import timeline_cases as tc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib

pytestmark = pytest.mark.gpu

KNOBS = ("freq_chunk_atoms", "freq_cap_items", "freq_frame_bits", "timeline_cap_bytes", "similarity_cap_bytes", "cluster_cap_bytes")
ARRAYS = set(cc.PER_SET + cc.PER_CLUSTER) | {"n_clusters", "n_total_frames"}


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


# ---- arp_bit_cluster: the kernels on bitmaps -------------------------------------------------------------------------------------------------------------
def check_bitmap(masks: np.ndarray, axes=cc.AXES, thresholds=None, max_clusters=None, words=None, what=""):
    """Device == host == numpy on the bytes of every output."""
    masks = np.asarray(masks, bool)
    n_bits = masks.shape[1]
    words = tc.pack(masks) if words is None else words
    for axis in axes:
        for thr in (cc.thresholds(masks, axis) if thresholds is None else thresholds):
            got = aa.bit_cluster(words, n_bits, thr, axis, max_clusters, device=0)
            cc.assert_clusters(got, cc.expected(masks, axis, thr, max_clusters), (what, axis, thr, max_clusters))
            assert to_bytes(got) == to_bytes(aa.bit_cluster(words, n_bits, thr, axis, max_clusters)), (what, axis, thr)


@pytest.mark.parametrize("M", cc.ROWS_M)
def test_word_and_tile_edges(ctx, M):
    """The word rows clustered (no transpose): M around every neighbour-word and tile edge, K at 1 word, a chunk less a word, a chunk, a chunk and a word, two
    chunks and a word, each with a full and with a partial last word; thresholds 0, 1 and two attained values."""
    cc.check_shape_reach()
    for K in cc.ROWS_K:
        for n_bits in sc.gram_bits(K):
            check_bitmap(sc.pattern("random0.5", M, n_bits, seed=M * 131 + n_bits), ("rows",), what=(M, K, n_bits))


@pytest.mark.parametrize("R", cc.TRANSPOSE_R)
def test_transpose_edges(ctx, R):
    """The bit columns clustered (k_bit_transpose in front, k_cluster_counts behind): rows around one, two and three 32-row tiles, frames from one bit to 33 words."""
    for F in cc.TRANSPOSE_F:
        check_bitmap(sc.pattern("random0.5", R, F, seed=R * 977 + F), ("frames",), what=(R, F))


@pytest.mark.parametrize("density", [0.01, 0.99])
def test_sparse_and_dense(ctx, density):
    for R, F in ((33, 65), (100, 197), (65, 1025)):
        check_bitmap(sc.pattern(f"random{density}", R, F, seed=R + F), what=(density, R, F))


def test_phantom_neighbours(ctx):
    """All ones at M = 33 and 65: every set has M neighbours, not 64 or 128 -- rows and columns past M are zero bits.  All zeros: empty unions are 1.0."""
    for M in (33, 65):
        for kind in ("ones", "zeros"):
            for sets, axis in ((sc.pattern(kind, M, 40), "rows"), (sc.pattern(kind, 40, M), "frames")):
                got = aa.bit_cluster(tc.pack(sets), sets.shape[1], 1.0, axis, device=0)
                assert (got["n_neighbours"] == M).all() and got["n_clusters"] == 1 and got["cluster_size"].tolist() == [M] and got["centre"].tolist() == [0]
                check_bitmap(sets, (axis,), (0.0, 0.5, 1.0), what=(kind, M, axis))


def test_dirty_bits_past_the_end(ctx):
    for R, F in ((1, 1), (5, 40), (sc.TILE + 1, 32 * sc.CHUNK - sc.GRAM_TAIL), (33, 65), (100, 1025 - 32 + 7)):
        m = sc.pattern("random0.5", R, F, seed=R + F)
        words = sc.dirty(tc.pack(m), F)
        assert not np.array_equal(words, tc.pack(m))
        check_bitmap(m, words=words, what=("dirty", R, F))


def test_mirror_is_a_transpose(ctx):
    """The staircase at 1/2: neighbour tiles (0, 1) and (1, 0) differ and neither is symmetric, so a mirror written without transposing (or not at all) shows."""
    sets, thr = cc.case_staircase()
    check_bitmap(sets, thresholds=(thr, 0.9), what="staircase")
    check_bitmap(sets.T, thresholds=(thr,), what="staircase T")


def test_thresholds(ctx):
    """0: one cluster, centre 0.  1: the groups of identical sets, empty sets together.  An attained value passes; the next f32 above it does not."""
    g = cc.case_identical_groups(empty=2)
    for sets, axis in ((g, "rows"), (g.T, "frames")):
        got = aa.bit_cluster(tc.pack(sets), sets.shape[1], 0.0, axis, device=0)
        assert got["n_clusters"] == 1 and got["centre"].tolist() == [0] and not got["cluster"].any()
        got = aa.bit_cluster(tc.pack(sets), sets.shape[1], 1.0, axis, device=0)
        assert got["n_clusters"] == 6 and all((g[got["cluster"] == k] == g[got["centre"][k]]).all() for k in range(6))
        check_bitmap(sets, (axis,), (0.0, 1.0), what="groups")
    sets, at, above = cc.case_attained()
    for s, axis in ((sets, "rows"), (sets.T, "frames")):
        assert aa.bit_cluster(tc.pack(s), s.shape[1], at, axis, device=0)["cluster"].tolist() == [0, 0, 1]
        assert aa.bit_cluster(tc.pack(s), s.shape[1], above, axis, device=0)["cluster"].tolist() == [0, 1, 2]
        check_bitmap(s, (axis,), (at, above), what="attained")


def test_ties_go_to_the_smaller_index(ctx):
    sets, thr = cc.case_tie()
    for s, axis in ((sets, "rows"), (sets.T, "frames")):
        got = aa.bit_cluster(tc.pack(s), s.shape[1], thr, axis, device=0)
        assert got["centre"].tolist() == [1, 3] and got["cluster"].tolist() == [0, 0, 0, 1]
        check_bitmap(s, (axis,), (thr,), what="tie")


def test_counts_run_over_the_frames_alive_now(ctx):
    """Three neighbourhoods in a chain: the frame with the second-highest initial degree has lost its neighbours to the first cluster."""
    sets, thr = cc.case_alive_counts()
    wrong, _, _ = cc.gromos(cc.adjacency(sets, "rows", thr)[0], recount=False)
    for s, axis in ((sets, "rows"), (sets.T, "frames")):
        got = aa.bit_cluster(tc.pack(s), s.shape[1], thr, axis, device=0)
        assert not np.array_equal(got["cluster"], wrong) and got["centre"].tolist()[:2] == [0, 8]
        check_bitmap(s, (axis,), (thr,), what="alive")


def test_singleton_tail(ctx):
    """65 distinct sets at 1.0: 65 clusters in index order (more than one tile; one launch of k_cluster_tail)."""
    sets = cc.case_distinct(65)
    for s, axis in ((sets, "rows"), (sets.T, "frames")):
        got = aa.bit_cluster(tc.pack(s), s.shape[1], 1.0, axis, device=0)
        assert got["n_clusters"] == 65 and got["centre"].tolist() == list(range(65)) and got["cluster"].tolist() == list(range(65))
        check_bitmap(s, (axis,), (1.0,), what="distinct")
        check_bitmap(s, (axis,), (1.0,), 40, what="distinct, capped in the tail")
    g, d = cc.case_identical_groups(), cc.case_distinct(300)  # four rounds for the groups, then a tail that starts behind them
    mixed = np.zeros((len(g) + len(d), g.shape[1] + d.shape[1]), bool)
    mixed[:len(g), :g.shape[1]], mixed[len(g):, g.shape[1]:] = g, d
    check_bitmap(mixed, ("rows",), (1.0,), what="groups + tail")
    check_bitmap(mixed.T, ("frames",), (1.0,), 200, what="groups + tail, capped")


@pytest.mark.parametrize("cap", [1, 2, 5, 6])
def test_max_clusters(ctx, cap):
    """Five clusters: the frames left over carry ARP_NONE and the NaN bits, the counts have min(cap, 5) columns."""
    g = cc.case_identical_groups()
    check_bitmap(g, ("rows",), (1.0,), cap, what=cap)
    check_bitmap(g.T, ("frames",), (1.0,), cap, what=cap)
    got = aa.bit_cluster(tc.pack(g.T), g.shape[0], 1.0, "frames", cap, device=0)
    left = got["cluster"] == cc.NONE
    assert got["cluster_counts"].shape == (g.shape[1], min(cap, 5)) and left.sum() == 15 - sum([5, 4, 3, 2, 1][:cap])
    assert (got["similarity_to_centre"].view("<u4")[left] == cc.NAN_BITS).all()


def test_cluster_counts(ctx):
    """np.add.at on the reference assignment; the row sums are the rows' frames; more clusters than one histogram sweep holds."""
    m = sc.pattern("random0.5", 40, 300, seed=4)
    words = tc.pack(m)
    for thr in cc.thresholds(m, "frames")[1:]:
        got = aa.bit_cluster(words, 300, thr, "frames", device=0)
        want = np.zeros((40, got["n_clusters"]), "<u4")
        r, f = np.nonzero(m)
        np.add.at(want, (r, cc.expected(m, "frames", thr)["cluster"][f]), 1)
        assert got["cluster_counts"].tobytes() == want.tobytes() and np.array_equal(got["cluster_counts"].sum(1), m.sum(1))
    F = cc.TAIL * cc.WORD + 70  # every frame another set: more singletons than one step of k_cluster_tail takes, and than two histogram sweeps hold
    big = np.zeros((3, F), bool)
    big[0] = True
    big[1, ::2] = True
    sets = ((np.arange(1, F + 1)[:, None] >> np.arange(14)[None, :]) & 1).astype(bool).T
    m = np.concatenate([big, sets])
    got = aa.bit_cluster(tc.pack(m), F, 1.0, "frames", device=0)
    assert got["n_clusters"] == F > 2 * cc.COUNT_TILE and got["cluster"].tolist() == list(range(F)) and got["centre"].tolist() == list(range(F))
    assert np.array_equal(got["cluster_counts"], m.astype("<u4")) and (got["n_neighbours"] == 1).all() and (got["similarity_to_centre"] == 1.0).all()


def test_bitmap_capacity(ctx):
    m = sc.pattern("random0.5", 10, 40)
    need = 40 * 2 * 4
    aa.debug_set("cluster_cap_bytes", need - 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        aa.bit_cluster(tc.pack(m), 40, 0.5, "frames", device=0)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "40 frames" in str(e.value) and f"{need} bytes" in str(e.value) and "cluster_cap_bytes" in str(e.value)
    check_bitmap(m, ("rows",), (0.4,))  # 10 x 1 words fit
    aa.debug_set("cluster_cap_bytes", need)
    aa.debug_set("similarity_cap_bytes", 1)  # (not this call's limit)
    check_bitmap(m, ("frames",), (0.4,))


# ---- end to end: closed-form schedules -------------------------------------------------------------------------------------------------------------------
def run(ctx, c: tc.Case, thr, **kw) -> dict:
    s = aa.Structure.from_records(c.top.rec)
    assert s.n_atoms == c.top.n
    aa.debug_set("freq_chunk_atoms", c.chunk_atoms)
    return ctx.contact_clusters(s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF, min_similarity=thr, **kw)


def assert_result(got: dict, masks: np.ndarray, thr, max_clusters=None, what="", counts=True):
    want = cc.expected(masks, "frames", thr, max_clusters, counts)
    cc.assert_clusters(got, want, what)
    assert got["n_total_frames"] == masks.shape[1]
    if counts and got["n_clusters"] and not (got["cluster"] == cc.NONE).any():
        assert np.array_equal(got["cluster_counts"].sum(1), got["n_frames"])
    assert got["cluster_size"].sum() == (got["cluster"] != cc.NONE).sum()


@pytest.mark.parametrize("name", ["frames_1", "frames_33", "frames_2049", "passes_gap"])
def test_closed_form(ctx, name):
    """The clusters of a schedule equal numpy on the schedule's masks (F = 1, 33, 2049; frames without any contact), the frequency columns are the closed form's."""
    sc.check_reach(name)
    c, masks, want = tc.cases()[name], sc.masks_of(name), tc.expected_of(name)
    for thr in cc.thresholds(masks, "frames"):
        got = run(ctx, c, thr)
        assert_result(got, masks, thr, what=(name, thr))
        assert set(got) == set(fe.COLUMNS) | ARRAYS | {"cluster_counts"}
        fe.assert_same_table({k: got[k] for k in fe.COLUMNS}, {k: want[k] for k in fe.COLUMNS})
    assert_result(run(ctx, c, 1.0, max_clusters=1), masks, 1.0, 1, (name, "capped"))


@pytest.mark.parametrize("name", ["frames_33", "passes_gap"])
def test_closed_form_residue_level(ctx, name):
    """Every atom of these topologies is a residue of its own: the residue-level rows are the atom-level rows in some order, which contact_timelines serves."""
    c = tc.cases()[name]
    s = aa.Structure.from_records(c.top.rec)
    tl = ctx.contact_timelines(s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF, level="residue")
    res_masks = aa.unpack_timeline(tl["timeline_words"], c.F)
    assert sorted(map(bytes, res_masks)) == sorted(map(bytes, sc.masks_of(name)))
    for thr in cc.thresholds(res_masks, "frames"):
        got = run(ctx, c, thr, level="residue")
        assert_result(got, res_masks, thr, what=(name, thr))
        assert got["from_residue"].tobytes() == tl["from_residue"].tobytes()


@pytest.mark.parametrize("level", ["atom", "residue"])
def test_no_contact_in_any_frame(ctx, level):
    """R = 0: every frame is the empty set, all are mutual neighbours at any threshold: one cluster with centre 0."""
    top, D = sc.no_contact_case(40)
    s = aa.Structure.from_records(top.rec)
    for thr in (0.0, 0.5, 1.0):
        got = ctx.contact_clusters(s, fe.frames(top, D), "/", fe.VDW_COMP, fe.CUTOFF, level=level, min_similarity=thr)
        assert_result(got, np.zeros((0, 40), bool), thr, what=("empty", thr))
        assert got["n_clusters"] == 1 and got["centre"].tolist() == [0] and got["cluster_size"].tolist() == [40] and got["cluster_counts"].shape == (0, 1)
        assert len(got["n_frames"]) == 0 and (got["n_neighbours"] == 40).all() and (got["similarity_to_centre"] == 1.0).all()


@pytest.mark.parametrize("level", ["atom", "residue"])
def test_pass_sizes(ctx, level):
    """The same schedule in passes of 5 and 33 frames (and, residue level, with 3 frame bits: 7 frames a pass) and in one pass: identical bytes."""
    c = tc.cases()["passes_dense"]
    thr = cc.thresholds(sc.masks_of("passes_dense"), "frames")[2]
    seen = {to_bytes(run(ctx, c.with_per(per), thr, level=level)) for per in (5, 33, None)}
    if level == "residue":
        aa.debug_set("freq_frame_bits", 3)
        seen.add(to_bytes(run(ctx, c, thr, level=level)))
    assert len(seen) == 1
    if level == "atom":
        assert_result(run(ctx, c.with_per(5), thr), sc.masks_of("passes_dense"), thr)


def test_capacity(ctx):
    """cluster_cap_bytes one byte below the neighbour bits' need is ARP_ERR_CAPACITY with F and the bytes in the message, before the marks sweep (the bitmap's
    own refusal would come there); at the need the call runs, and similarity_cap_bytes below F x F x 4 does not concern it."""
    name = "passes_dense"
    c, masks = tc.cases()[name], sc.masks_of(name)
    need = c.F * c.W * 4
    aa.debug_set("cluster_cap_bytes", need - 1)
    aa.debug_set("timeline_cap_bytes", 1)
    with pytest.raises(aa.ArpeggiaError) as e:
        run(ctx, c, 0.5)
    assert e.value.status == _lib.ARP_ERR_CAPACITY
    for part in (f"{c.F} frames", f"{need} bytes", "cluster_cap_bytes"):
        assert part in str(e.value), str(e.value)
    aa.debug_set("cluster_cap_bytes", need)
    with pytest.raises(aa.ArpeggiaError) as e:
        run(ctx, c, 0.5)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "timeline_cap_bytes" in str(e.value)  # the bitmap's own limit still applies, later
    aa.debug_set("timeline_cap_bytes", 0)
    aa.debug_set("similarity_cap_bytes", c.F * c.F * 4 - 1)
    with pytest.raises(aa.ArpeggiaError):
        ctx.contact_similarity(aa.Structure.from_records(c.top.rec), fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF)
    assert_result(run(ctx, c, 0.5), masks, 0.5)  # the ground the similarity route cannot cover


def test_counts_capacity_and_no_counts(ctx, ubq_path):
    """Thousands of rows, eight frames: the neighbour bits are 32 bytes, the counts are refused under a limit of 64 -- and are not needed with counts=False,
    which gives the same other bytes."""
    s = aa.load_model(ubq_path)
    frames = jittered(s, 8, seed=3)
    full = ctx.contact_clusters(s, frames, "/", min_similarity=1.0)
    assert full["n_clusters"] == 8 and full["cluster_counts"].shape == (len(full["n_frames"]), 8)
    aa.debug_set("cluster_cap_bytes", 64)
    with pytest.raises(aa.ArpeggiaError) as e:
        ctx.contact_clusters(s, frames, "/", min_similarity=1.0)
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "counts" in str(e.value) and f"{len(full['n_frames']) * 8 * 4} bytes" in str(e.value)
    bare = ctx.contact_clusters(s, frames, "/", min_similarity=1.0, counts=False)
    assert "cluster_counts" not in bare and to_bytes(bare) == to_bytes({k: v for k, v in full.items() if k != "cluster_counts"})


def test_table_handle(ctx):
    """arp_table_clusters serves the arrays of a cluster table and NULL for every other table; the cluster table has no timeline columns."""
    c = tc.cases()["passes_gap"]
    s = aa.Structure.from_records(c.top.rec)
    xyz = fe.frames(c.top, c.D)
    for counts in (True, False):
        t = aa.api._cluster_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF, False, "atom", 0.5, None, counts)
        try:
            m, n, flags, cnt = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.POINTER(C.c_uint32)()
            assert lib.arp_table_clusters(t, C.byref(m), C.byref(n), C.byref(flags), None, None, None, None, None, C.byref(cnt)) is not None
            assert m.value == c.F and n.value >= 1 and flags.value == (0 if counts else _lib.ARP_CLUSTER_NO_COUNTS) and bool(cnt) == counts
            assert lib.arp_table_clusters(t, *([None] * 9)) is not None
            assert lib.arp_table_timeline(t, None, None) is None and lib.arp_table_similarity(t, None, None, None) is None
        finally:
            lib.arp_table_free(t)
    for other in (aa.api._freq_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF), aa.api._similarity_table(ctx, s, xyz, "/", fe.VDW_COMP, fe.CUTOFF, False, "atom", "frames", "tanimoto")):
        try:
            assert lib.arp_table_clusters(other, *([None] * 9)) is None
        finally:
            lib.arp_table_free(other)


# ---- end to end: natural inputs ---------------------------------------------------------------------------------------------------------------------------
def jittered(s: aa.Structure, n_frames: int, seed: int, sigma: float = 0.3) -> np.ndarray:
    n = aa.api._topology_atoms(s)
    soa = s.soa("/")
    xyz = np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)
    return xyz[None] + np.random.default_rng(seed).normal(scale=sigma, size=(n_frames, n, 3))


def want_from_calls(ctx, s, frames, groups, rings, level, thr, max_clusters=None) -> dict:
    """The reference run on the matrix of contact_similarity; the counts from the bitmap of contact_timelines."""
    sim = ctx.contact_similarity(s, frames, groups, rings=rings, level=level)
    adj = sim["similarity"] >= np.float32(thr)
    cluster, centre, size = cc.gromos(adj, max_clusters)
    F = len(adj)
    got = cluster != cc.NONE
    to_centre = np.full(F, cc.NAN_BITS, "<u4").view("<f4")
    to_centre[got] = sim["similarity"][np.arange(F)[got], centre[cluster[got]]]
    masks = aa.unpack_timeline(ctx.contact_timelines(s, frames, groups, rings=rings, level=level)["timeline_words"], F)
    counts = np.zeros((masks.shape[0], len(centre)), "<u4")
    r, f = np.nonzero(masks[:, got])
    np.add.at(counts, (r, cluster[got][f]), 1)
    return {"cluster": cluster, "similarity_to_centre": to_centre, "n_neighbours": adj.sum(1).astype("<u4"), "sizes": sim["sizes"], "centre": centre, "cluster_size": size,
            "n_clusters": len(centre), "cluster_counts": counts}, sim["similarity"]


def check_natural(ctx, s, frames, groups, per: int, rings: bool = False):
    F, n = frames.shape[0], frames.shape[1]
    n_clusters = set()
    for level in ("atom", "residue"):
        fq = ctx.contact_frequencies(s, frames, groups, rings=rings, level=level)
        sim = ctx.contact_similarity(s, frames, groups, rings=rings, level=level)["similarity"]
        off = np.sort(sim[~np.eye(F, dtype=bool)])
        for thr, cap in ((float(off[len(off) // 2]), None), (float(off[(len(off) * 9) // 10]), None), (float(off[(len(off) * 9) // 10]), 3)):
            want, _ = want_from_calls(ctx, s, frames, groups, rings, level, thr, cap)
            got = ctx.contact_clusters(s, frames, groups, rings=rings, level=level, min_similarity=thr, max_clusters=cap)
            cc.assert_clusters(got, want, (level, thr, cap))
            assert set(fq) <= set(got) and set(got) - set(fq) == ARRAYS | {"cluster_counts"}
            for col in fq:
                assert got[col].dtype == fq[col].dtype and got[col].tobytes() == fq[col].tobytes(), col
            n_clusters.add(got["n_clusters"])
        assert to_bytes(ctx.contact_clusters(s, frames, groups, rings=rings, level=level, min_similarity=thr, max_clusters=cap)) == to_bytes(got)  # repeatable
        assert F % per and -(-F // per) >= 3
        aa.debug_set("freq_chunk_atoms", per * n)
        assert to_bytes(ctx.contact_clusters(s, frames, groups, rings=rings, level=level, min_similarity=thr, max_clusters=cap)) == to_bytes(got)
        aa.debug_set("freq_chunk_atoms", 0)
    return n_clusters


def test_ubq_70_frames(ctx, ubq_path):
    s = aa.load_model(ubq_path)
    assert max(check_natural(ctx, s, jittered(s, 70, seed=71), "/", per=25)) > 3


def test_bft_16_frames_chain_groups(ctx, bft_path):
    s = aa.load_model(bft_path)
    check_natural(ctx, s, jittered(s, 16, seed=21), "H,L/C", per=5)


def test_ring_topology(ctx):
    """A ring topology of freq_ring_cases, rings on: the ring rows take part in the frames' sets and in the counts."""
    case = rg.build("clusters", ["rr"] * 3 + ["rc"] * 2 + ["alt"] + ["rr"] + ["rc"], F=38, pads=20)
    s = aa.Structure.from_records(case.rec)
    check_natural(ctx, s, case.frames, "/", per=7, rings=True)
    plain = ctx.contact_clusters(s, case.frames, "/", min_similarity=0.5)
    with_rings = ctx.contact_clusters(s, case.frames, "/", rings=True, min_similarity=0.5)
    assert (plain["sizes"] <= with_rings["sizes"]).all() and (plain["sizes"] < with_rings["sizes"]).any()


def test_model_file(ctx, tmp_path, ubq_path):
    """A MODEL-record file with frames=None: the models are the frames; contact_clusters(path) and the command line give the same clusters and the frequency
    call's table."""
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
    sim = ctx.contact_similarity(s, None, "/")["similarity"]
    thr = float(np.sort(sim[~np.eye(F, dtype=bool)])[F * (F - 1) // 2])
    from_models = ctx.contact_clusters(s, None, "/", min_similarity=thr)
    assert from_models["n_total_frames"] == F and to_bytes(from_models) == to_bytes(ctx.contact_clusters(s, frames, "/", min_similarity=thr))
    want, _ = want_from_calls(ctx, s, None, "/", False, "atom", thr)
    cc.assert_clusters(from_models, want, "models")
    assert to_bytes(aa.contact_clusters(str(path), min_similarity=thr)) == to_bytes(from_models)
    assert to_bytes(aa.get_contact_clusters(s, None, "/", min_similarity=thr, max_clusters=1)) == to_bytes(ctx.contact_clusters(s, frames, "/", min_similarity=thr, max_clusters=1))
    import pyarrow.parquet as pq

    assert main(["contact-clusters", "-i", str(path), "-o", str(tmp_path), "-t", "parquet", "--min-similarity", repr(thr), "--assignments", str(tmp_path / "a.csv"),
                 "--cluster-counts", str(tmp_path / "cc.npy")]) == 0
    table = pq.read_table(str(tmp_path / "contact_clusters.parquet"))
    assert table.column_names == [c for c, _ in aa.FREQ_COLUMNS]
    freq = aa.get_contact_frequencies(s, None, "/")
    freq = freq if hasattr(freq, "column_names") else freq.to_arrow()
    for c in freq.column_names:
        assert table.column(c).to_pylist() == freq.column(c).to_pylist(), c
    # (the command line parses the threshold as a Python float and hands it on as f32, as every layer does)
    saved = np.load(tmp_path / "cc.npy")
    assert saved.dtype == np.uint32 and saved.tobytes() == from_models["cluster_counts"].tobytes()
    lines = (tmp_path / "a.csv").read_text().splitlines()
    assert lines[0] == "frame,cluster,is_centre,similarity_to_centre,n_neighbours,size" and len(lines) == F + 1
    for k, line in enumerate(lines[1:]):
        f, cl, is_c, st, nn, size = line.split(",")
        assert (int(f), int(cl), int(nn), int(size)) == (k, from_models["cluster"][k], from_models["n_neighbours"][k], from_models["sizes"][k])
        assert (is_c == "1") == (k in from_models["centre"].tolist()) and np.float32(float(st)) == from_models["similarity_to_centre"][k]
    assert main(["contact-clusters", "-i", str(path), "-o", str(tmp_path), "--min-similarity", "1", "--max-clusters", "1", "--assignments", str(tmp_path / "b.csv")]) == 0
    assert sum(line.split(",")[1] == "" for line in (tmp_path / "b.csv").read_text().splitlines()[1:]) == F - 1
    assert main(["contact-clusters", "-i", str(path), "-o", str(tmp_path), "--min-similarity", "1.5"]) == 1
