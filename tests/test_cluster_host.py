"""Contact clusters: everything that needs no device.  arp_bit_cluster_host (the restatement of the definition on the CPU, and the yardstick of
k_bit_adjacency / k_cluster_round / k_cluster_tail / k_cluster_counts) against plain numpy; every case's reach assertions; the checks arp_contact_clusters
runs before the device is touched; the exports; the CLI's flags."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import cluster_cases as cc
import similarity_cases as sc
import timeline_cases as tc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib


def refused(status: int, fn, *args, match: str | None = None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)
    return str(e.value)


def check_host(masks: np.ndarray, axes=cc.AXES, thresholds=None, max_clusters=None, words=None, what=""):
    masks = np.asarray(masks, bool)
    words = tc.pack(masks) if words is None else words
    for axis in axes:
        for thr in (cc.thresholds(masks, axis) if thresholds is None else thresholds):
            got = aa.bit_cluster(words, masks.shape[1], thr, axis, max_clusters)
            cc.assert_clusters(got, cc.expected(masks, axis, thr, max_clusters), (what, axis, thr, max_clusters))


def test_exported():
    header = (Path(aa.__file__).resolve().parent.parent / "include" / "arpeggia_amd.h").read_text()
    for name in ("arp_contact_clusters", "arp_table_clusters", "arp_bit_cluster_host", "arp_bit_cluster"):
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\(", header), name
    assert lib.arp_api_version() == 2  # additive exports do not move the layout version
    assert re.search(rf"#define ARP_CLUSTER_NO_COUNTS {_lib.ARP_CLUSTER_NO_COUNTS:#x}u\b", header) and _lib.ARP_CLUSTER_NO_COUNTS == 0x40
    flags = [_lib.ARP_FREQ_RINGS, _lib.ARP_TIMELINE_NO_BITMAP, _lib.ARP_SIM_COUNTS, _lib.ARP_SIM_ROWS, _lib.ARP_ACF_CONTINUOUS, _lib.ARP_ACF_NO_MATRIX, _lib.ARP_CLUSTER_NO_COUNTS]
    assert len(set(flags)) == 7 and all(f & (f - 1) == 0 for f in flags)  # seven different bits
    for word in ("cluster_cap_bytes", "min_similarity", "max_clusters", "similarity_to_centre", "n_neighbours", "cluster_counts", "gromos"):
        assert word in header, word
    for name in ("bit_cluster", "contact_clusters", "get_contact_clusters"):
        assert callable(getattr(aa, name))
    assert callable(aa.Context.contact_clusters)


def test_cases_reach_their_mechanisms():
    cc.check_directed_reach()


def test_reference_by_hand():
    """The numpy reference itself on sets small enough to do by hand: {0, 1}, {1, 2}, {3}, {}, {} at 1/3 and at 1."""
    sets = np.zeros((5, 4), bool)
    sets[0, [0, 1]] = sets[1, [1, 2]] = True
    sets[2, 3] = True
    w = cc.expected(sets, "rows", np.float32(1 / 3))
    assert w["cluster"].tolist() == [0, 0, 2, 1, 1] and w["centre"].tolist() == [0, 3, 2] and w["cluster_size"].tolist() == [2, 2, 1]
    assert w["n_neighbours"].tolist() == [2, 2, 1, 2, 2] and w["sizes"].tolist() == [2, 2, 1, 0, 0]
    assert w["similarity_to_centre"].tolist() == [1.0, np.float32(1 / 3), 1.0, 1.0, 1.0]
    w = cc.expected(sets, "rows", 1.0)
    assert w["cluster"].tolist() == [1, 2, 3, 0, 0] and w["centre"].tolist() == [3, 0, 1, 2]
    w = cc.expected(sets.T, "frames", 1.0, max_clusters=2)
    assert w["cluster"].tolist() == [1, cc.NONE, cc.NONE, 0, 0] and w["cluster_counts"].tolist() == [[0, 1], [0, 1], [0, 0], [0, 0]]
    assert w["similarity_to_centre"].view("<u4").tolist()[1:3] == [cc.NAN_BITS] * 2


@pytest.mark.parametrize("rows", cc.HOST_ROWS)
@pytest.mark.parametrize("n_bits", cc.HOST_BITS)
def test_host_shapes(n_bits, rows):
    """Every rows x n_bits of the lists, both axes, three densities; thresholds 0, 1 and two attained values of the bitmap itself."""
    for density in cc.DENSITIES:
        check_host(sc.pattern(f"random{density}", rows, n_bits, seed=rows * 10007 + n_bits), what=(rows, n_bits, density))


@pytest.mark.parametrize("kind", ["zeros", "ones"])
def test_host_uniform(kind):
    for rows, n_bits in ((1, 1), (2, 33), (33, 65), (65, 1025), (31, 64)):
        m = sc.pattern(kind, rows, n_bits)
        check_host(m, what=(kind, rows, n_bits))
        for axis in cc.AXES:
            got = aa.bit_cluster(tc.pack(m), n_bits, 1.0, axis)
            M = rows if axis == "rows" else n_bits
            assert got["n_clusters"] == 1 and got["centre"].tolist() == [0] and got["cluster_size"].tolist() == [M] and (got["n_neighbours"] == M).all()
            assert (got["similarity_to_centre"] == 1.0).all()


def test_bits_past_the_end_are_ignored():
    for rows, n_bits in ((1, 1), (5, 40), (33, 65), (2, 1023)):
        m = sc.pattern("random0.5", rows, n_bits, seed=3)
        words = sc.dirty(tc.pack(m), n_bits)
        assert not np.array_equal(words, tc.pack(m))
        check_host(m, words=words, what=("dirty", rows, n_bits))


def test_thresholds():
    """0: one cluster around set 0.  1: the groups of identical sets, the empty ones together.  An attained value passes, the next f32 above it does not."""
    g = cc.case_identical_groups(empty=2)
    for sets, axis in ((g, "rows"), (g.T, "frames")):
        got = aa.bit_cluster(tc.pack(sets), sets.shape[1], 0.0, axis)
        assert got["n_clusters"] == 1 and got["centre"].tolist() == [0] and not got["cluster"].any()
        got = aa.bit_cluster(tc.pack(sets), sets.shape[1], 1.0, axis)
        assert got["n_clusters"] == 6 and (got["similarity_to_centre"] == 1.0).all()
        for k in range(6):
            members = g[got["cluster"] == k]
            assert (members == members[0]).all()
        check_host(sets, (axis,), (0.0, 1.0))
    sets, at, above = cc.case_attained()
    for s, axis in ((sets, "rows"), (sets.T, "frames")):
        assert aa.bit_cluster(tc.pack(s), s.shape[1], at, axis)["cluster"].tolist() == [0, 0, 1]
        assert aa.bit_cluster(tc.pack(s), s.shape[1], above, axis)["cluster"].tolist() == [0, 1, 2]
        check_host(s, (axis,), (at, above))


def test_directed_cases():
    """Ties to the smaller index; counts over the frames alive now; the singleton tail; max_clusters; the staircase."""
    for sets, thr in (cc.case_tie(), cc.case_alive_counts(), cc.case_staircase(), (cc.case_distinct(), 1.0)):
        check_host(sets, ("rows",), (thr,))
        check_host(sets.T, ("frames",), (thr,))
    sets, thr = cc.case_alive_counts()
    wrong, _, _ = cc.gromos(cc.adjacency(sets, "rows", thr)[0], recount=False)
    assert not np.array_equal(aa.bit_cluster(tc.pack(sets), sets.shape[1], thr, "rows")["cluster"], wrong)
    g = cc.case_identical_groups()
    for cap in (1, 2, 5, 6):
        check_host(g, ("rows",), (1.0,), cap)
        check_host(g.T, ("frames",), (1.0,), cap)
    got = aa.bit_cluster(tc.pack(g.T), g.shape[0], 1.0, "frames", 2)
    assert got["cluster_counts"].shape == (g.shape[1], 2) and (got["cluster"] == cc.NONE).sum() == 6
    assert (got["similarity_to_centre"].view("<u4")[got["cluster"] == cc.NONE] == cc.NAN_BITS).all()


def test_empty_bitmaps():
    got = aa.bit_cluster(np.zeros((0, 2), "<u4"), 40, 0.5, "rows")
    assert got["n_clusters"] == 0 and got["cluster"].shape == (0,) and got["centre"].shape == (0,)
    got = aa.bit_cluster(np.zeros((0, 2), "<u4"), 40, 0.5, "frames")  # 40 empty sets: all mutual neighbours, one cluster around frame 0
    assert got["n_clusters"] == 1 and got["centre"].tolist() == [0] and got["cluster_size"].tolist() == [40] and got["cluster_counts"].shape == (0, 1)
    assert (got["n_neighbours"] == 40).all() and (got["similarity_to_centre"] == 1.0).all() and not got["sizes"].any()
    got = aa.bit_cluster(np.ones((1, 1), "<u4"), 1, 1.0, "frames")
    assert got["n_clusters"] == 1 and got["cluster"].tolist() == [0] and got["cluster_counts"].tolist() == [[1]]


def raw(fn, ctx, rows, n_bits, words, flags, thr, cap, null=None, counts=False):
    """arp_bit_cluster_host / arp_bit_cluster with raw pointers; `null` names the argument passed as NULL."""
    M = rows if flags & _lib.ARP_SIM_ROWS else n_bits
    u32p, fp = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    room = min(max(M, 1), 64)  # (the calls that name more sets than this are refused before anything is written)
    bufs = {k: np.zeros(room * (min(rows, 64) if k == "counts" else 1), "<f4" if k == "sim" else "<u4") for k in ("cluster", "sim", "nn", "sizes", "centre", "csize", "n", "counts")}
    p = lambda k: None if k == null or (k == "counts" and not counts) else bufs[k].ctypes.data_as(fp if k == "sim" else u32p)
    w = None if null == "words" else words.ctypes.data_as(u32p)
    args = (rows, n_bits, w, flags, C.c_float(thr), cap, p("cluster"), p("sim"), p("nn"), p("sizes"), p("centre"), p("csize"), p("n"), p("counts"))
    return fn(*args) if ctx is None else fn(ctx, *args)


def test_bad_arguments():
    words = np.zeros((2, 2), "<u4")
    host = lambda *a, **kw: aa.api._check(raw(lib.arp_bit_cluster_host, None, *a, **kw))
    for flags in (0, _lib.ARP_SIM_ROWS):
        assert raw(lib.arp_bit_cluster_host, None, 2, 40, words, flags, 0.5, _lib.ARP_NONE) == _lib.ARP_OK
        for thr in (float("nan"), -0.1, 1.5, float("inf"), -float("inf")):
            refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, words, flags, thr, _lib.ARP_NONE, match="min_similarity")
        refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, words, flags, 0.5, 0, match="max_clusters")
        for null in ("words", "cluster", "sim", "nn", "sizes", "centre", "csize", "n"):
            refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, words, flags, 0.5, 1, null=null, match="null")
        for bad in (_lib.ARP_SIM_COUNTS, _lib.ARP_FREQ_RINGS, _lib.ARP_CLUSTER_NO_COUNTS, 0x80000000):
            refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, words, flags | bad, 0.5, 1, match="unknown flag bits")
    refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, words, _lib.ARP_SIM_ROWS, 0.5, 1, counts=True, match="cluster_counts")
    assert raw(lib.arp_bit_cluster_host, None, 2, 40, words, 0, 0.5, 1, counts=True) == _lib.ARP_OK
    refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 1 << 32, words, _lib.ARP_SIM_ROWS, 0.5, 1, match="2^32")
    refused(_lib.ARP_ERR_BAD_INPUT, host, 1 << 32, 40, words, 0, 0.5, 1, match="2^32")
    assert lib.arp_bit_cluster(None, 2, 40, words.ctypes.data_as(C.POINTER(C.c_uint32)), 0, C.c_float(0.5), 1, *([None] * 8)) == _lib.ARP_ERR_BAD_INPUT  # no context
    for thr in (0.0, -0.0, 1.0):
        assert raw(lib.arp_bit_cluster_host, None, 2, 40, words, 0, thr, 1) == _lib.ARP_OK
    with pytest.raises(ValueError):
        aa.bit_cluster(words, 65, 0.5)
    with pytest.raises(ValueError):
        aa.bit_cluster(words, 40, 0.5, axis="columns")
    with pytest.raises(ValueError):
        aa.bit_cluster(words, 40, 0.5, max_clusters=-1)
    with pytest.raises(TypeError):
        aa.bit_cluster(words, 40)  # min_similarity has no default


# ---- what arp_contact_clusters decides before the device is touched -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


def frames_of(s: aa.Structure, F: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)[None].repeat(F, 0)


def checked(s, frames, groups="/", flags=0, level=0, thr=0.5, cap=_lib.ARP_NONE) -> int:
    """arp_contact_clusters with ctx == NULL: only the checks run."""
    n_frames, ptr, keep = aa.api._frames_arg(s, frames, "contact clusters")
    t = C.c_void_p(1)
    st = lib.arp_contact_clusters(None, s._h, int(n_frames), ptr, groups.encode(), 0.1, 6.5, flags, level, thr, cap, C.byref(t))
    if st == _lib.ARP_OK:
        assert t.value is None  # *out = NULL
    return st


def test_null_context_runs_only_the_checks(ubq):
    for flags in (0, _lib.ARP_FREQ_RINGS, _lib.ARP_CLUSTER_NO_COUNTS, _lib.ARP_FREQ_RINGS | _lib.ARP_CLUSTER_NO_COUNTS):
        for level in (0, 1):
            for thr, cap in ((0.0, 1), (1.0, _lib.ARP_NONE), (0.5, 7)):
                assert checked(ubq, frames_of(ubq, 2), flags=flags, level=level, thr=thr, cap=cap) == _lib.ARP_OK


@pytest.mark.parametrize("thr", [float("nan"), -0.1, 1.5, float("inf")])
def test_bad_min_similarity(ubq, thr):
    assert checked(ubq, frames_of(ubq, 1), thr=thr) == _lib.ARP_ERR_BAD_INPUT
    assert "min_similarity" in lib.arp_last_error().decode()
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_contact_clusters, ubq, frames_of(ubq, 1), min_similarity=thr, match="min_similarity")


def test_bad_max_clusters_and_missing_threshold(ubq):
    assert checked(ubq, frames_of(ubq, 1), cap=0) == _lib.ARP_ERR_BAD_INPUT
    assert "max_clusters" in lib.arp_last_error().decode()
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_contact_clusters, ubq, frames_of(ubq, 1), min_similarity=0.5, max_clusters=0, match="max_clusters")
    with pytest.raises(ValueError):
        aa.get_contact_clusters(ubq, frames_of(ubq, 1), min_similarity=0.5, max_clusters=-3)
    for fn, args in ((aa.get_contact_clusters, (ubq,)), (aa.contact_clusters, ("x.pdb",)), (aa.Context.contact_clusters, (None, ubq))):
        with pytest.raises(TypeError):
            fn(*args)  # min_similarity has no default in any layer


@pytest.mark.parametrize("level", [-1, 2, 7])
def test_bad_level(ubq, level):
    assert checked(ubq, frames_of(ubq, 1), level=level) == _lib.ARP_ERR_BAD_INPUT
    assert "level" in lib.arp_last_error().decode()
    with pytest.raises(ValueError):
        aa.get_contact_clusters(ubq, frames_of(ubq, 1), level="chain", min_similarity=0.5)


@pytest.mark.parametrize("flags", [_lib.ARP_SIM_ROWS, _lib.ARP_SIM_COUNTS, _lib.ARP_TIMELINE_NO_BITMAP, _lib.ARP_ACF_NO_MATRIX, 0x80, 0x80000000, 0x7F])
def test_unknown_flag(ubq, flags):
    assert checked(ubq, frames_of(ubq, 1), flags=flags) == _lib.ARP_ERR_BAD_INPUT
    assert "unknown flag bits" in lib.arp_last_error().decode()


@pytest.mark.parametrize("level", ["atom", "residue"])
def test_input_errors_are_those_of_the_frequency_call(ubq, level):
    """The frequency call's errors, with status and message, whatever the device -- and they come before the checks on the two new arguments."""
    def same(*args, **kw):
        out = []
        for fn, extra in ((aa.get_contact_frequencies, {}), (aa.get_contact_clusters, {"min_similarity": float("nan")})):
            with pytest.raises(aa.ArpeggiaError) as e:
                fn(*args, level=level, **kw, **extra)
            out.append((e.value.status, str(e.value)))
        assert out[0] == out[1] or (out[0][0] == out[1][0] and out[0][1].replace("contact frequencies", "contact clusters") == out[1][1]), out
        assert out[0][0] != _lib.ARP_ERR_NO_DEVICE
        return out[1][1]

    assert "at least one frame" in same(ubq, frames_of(ubq, 0))
    assert "shape" in same(ubq, np.zeros((2, 5, 3)))
    f = frames_of(ubq, 3)
    f[2, 17, 1] = np.nan
    assert "frame 2, atom 17" in same(ubq, f)
    for groups in ("", "A", "A/B/C,", "Z/", "/A"):
        try:
            aa.api.parse_groups(["A"], groups)
        except aa.ArpeggiaError:
            same(ubq, frames_of(ubq, 1), groups)


def test_cap_knob():
    aa.debug_set("cluster_cap_bytes", 1)
    aa.debug_set("cluster_cap_bytes", 1 << 40)
    aa.debug_set("cluster_cap_bytes", 0)
    refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "cluster_cap_bytes", -1)
    assert "cluster_cap_bytes" in refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "no_such_knob", 1)


def test_ten_to_the_five_frames_are_legal_by_the_arithmetic():
    F = 10 ** 5
    assert F * -(-F // 32) * 4 == 1_250_000_000 < 2 ** 31 < F * F * 4


def test_table_clusters_of_nothing():
    assert lib.arp_table_clusters(None, *([None] * 9)) is None


def test_cli_defaults_and_flags(tmp_path):
    from arpeggia_amd.__main__ import build_parser, main

    a = build_parser().parse_args(["contact-clusters", "-i", "x.pdb", "-o", str(tmp_path), "--min-similarity", "0.4"])
    assert (a.groups, a.filename, a.output_format, a.vdw_comp, a.dist_cutoff, a.num_threads, a.ignore_zero_occupancy, a.rings, a.level, a.min_similarity, a.max_clusters,
            a.assignments, a.cluster_counts) == ("/", "contact_clusters", "csv", 0.1, 6.5, 1, False, False, "atom", 0.4, None, None, None)
    assert not hasattr(a, "bitmap") and not hasattr(a, "axis") and not hasattr(a, "matrix")
    a = build_parser().parse_args(["contact-clusters", "-i", "x.pdb", "-o", "d", "-g", "A/B", "-f", "f", "-t", "PARQUET", "-c", "0.2", "-d", "5", "-j", "4",
                                   "--ignore-zero-occupancy", "--rings", "-l", "residue", "--min-similarity", "1", "--max-clusters", "3", "--assignments", "a.csv",
                                   "--cluster-counts", "c.npy"])
    assert (a.groups, a.filename, a.output_format, a.vdw_comp, a.dist_cutoff, a.num_threads, a.ignore_zero_occupancy, a.rings, a.level, a.min_similarity, a.max_clusters,
            str(a.assignments), str(a.cluster_counts)) == ("A/B", "f", "parquet", 0.2, 5.0, 4, True, True, "residue", 1.0, 3, "a.csv", "c.npy")
    for bad in ([], ["--min-similarity", "x"], ["--min-similarity", "0.5", "--axis", "rows"], ["--min-similarity", "0.5", "--max-clusters", "two"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["contact-clusters", "-i", "x.pdb", "-o", "d"] + bad)
    assert main(["contact-clusters", "-i", str(tmp_path / "none.pdb"), "-o", str(tmp_path), "--min-similarity", "0.5"]) == 1
