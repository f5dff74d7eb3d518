"""Contact autocorrelation on the CPU: arp_bit_autocorr_host (the definition, bit by bit) against the numpy references of tests/autocorr_cases.py, the
by-hand facts, every refusal that is decided before a device is touched, the exports, the flags and the command line's flags."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import autocorr_cases as ac
import similarity_cases as sc
import timeline_cases as tc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib


def refused(status, fn, *args, match=None, **kw) -> str:
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, (e.value.status, str(e.value))
    if match:
        assert match in str(e.value), str(e.value)
    return str(e.value)


def check_host(masks, L, what="", words=None, group=None, n_groups=0):
    masks = np.asarray(masks, bool)
    F = masks.shape[1]
    words = tc.pack(masks) if words is None else words
    out = {}
    for mode in ac.MODES:
        want = ac.reference(masks, L, mode, group, n_groups)
        got = aa.bit_autocorrelation(words, F, L, mode, group, n_groups)
        ac.assert_same(got, want, (what, mode))
        assert np.array_equal(got["lags"], np.arange(L + 1))
        out[mode] = got
    assert (out["continuous"]["autocorrelation"] <= out["intermittent"]["autocorrelation"]).all()
    assert np.array_equal(out["continuous"]["autocorrelation"][:, 0], masks.sum(1))
    return out


def test_exported_and_flags():
    header = (Path(aa.__file__).resolve().parent.parent / "include" / "arpeggia_amd.h").read_text()
    for name in ("arp_contact_autocorrelation", "arp_table_autocorrelation", "arp_bit_autocorr_host", "arp_bit_autocorr"):
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\(", header), name
    assert lib.arp_api_version() == 2  # additive exports do not move the layout version
    for name, value in (("ARP_ACF_CONTINUOUS", 0x10), ("ARP_ACF_NO_MATRIX", 0x20)):
        assert getattr(_lib, name) == value
        assert re.search(r"#define " + name + r" 0x%xu\b" % value, header), name
    six = [_lib.ARP_FREQ_RINGS, _lib.ARP_TIMELINE_NO_BITMAP, _lib.ARP_SIM_COUNTS, _lib.ARP_SIM_ROWS, _lib.ARP_ACF_CONTINUOUS, _lib.ARP_ACF_NO_MATRIX]
    assert len(set(six)) == 6 and all(f and f & (f - 1) == 0 for f in six)
    for name in ("bit_autocorrelation", "contact_autocorrelation", "get_contact_autocorrelation"):
        assert callable(getattr(aa, name))
    assert callable(aa.Context.contact_autocorrelation)


def test_cases_reach():
    """Every case reaches what it is named for, and the host function gives the reference's curves on the masks of every closed-form schedule."""
    ac.check_bitmap_reach()
    for name in ac.CLOSED:
        ac.check_reach(name)
        masks = ac.masks_of(name)
        check_host(masks, masks.shape[1] - 1, name, group=ac.codes_of(name), n_groups=ac.N_INTERACTIONS)


@pytest.mark.parametrize("rows", ac.HOST_ROWS)
def test_host_matches_numpy(rows):
    """rows x F x L (clipped to L < F), both modes: three densities, all ones, all zeros, alternating, one bit at frame 0 and at F - 1, a run over a word
    boundary."""
    for F in ac.HOST_BITS:
        for L in ac.host_lags(F):
            for kind in ac.PATTERNS:
                check_host(ac.pattern(kind, rows, F, seed=rows * 7 + F), L, (kind, rows, F, L))


@pytest.mark.parametrize("kind", [k for k in ac.PATTERNS if not k.startswith("random")])
def test_host_patterns(kind):
    for rows, F in ((1, 1), (2, 33), (2, 65), (3, 1025)):
        for L in {0, min(F - 1, 33), F - 1}:
            check_host(ac.pattern(kind, rows, F), L, (kind, rows, F, L))


def test_all_ones_by_hand():
    got = check_host(np.ones((2, 40), bool), 39)
    for mode in ac.MODES:
        assert got[mode]["autocorrelation"].tolist() == [[40 - t for t in range(40)]] * 2
        assert got[mode]["half_life"].tolist() == [ac.NONE] * 2  # the window-corrected estimator stays at 1


def test_alternating_by_hand():
    got = check_host(ac.pattern("alternating", 1, 40), 39)
    assert got["intermittent"]["autocorrelation"][0].tolist() == [20 - t // 2 if t % 2 == 0 else 0 for t in range(40)]
    assert got["intermittent"]["autocorrelation"][0, :5].tolist() == [20, 0, 19, 0, 18]
    assert got["intermittent"]["half_life"].tolist() == [1]
    assert got["continuous"]["autocorrelation"][0].tolist() == [20] + [0] * 39
    assert got["continuous"]["half_life"].tolist() == [1]


def test_max_lag_zero_and_default():
    m = ac.pattern("random0.5", 5, 70, seed=1)
    got = check_host(m, 0)
    for mode in ac.MODES:
        assert got[mode]["autocorrelation"].shape == (5, 1) and (got[mode]["half_life"] == ac.NONE).all()
    full = aa.bit_autocorrelation(tc.pack(m), 70)
    assert full["autocorrelation"].shape == (5, 70)
    ac.assert_same(full, ac.reference(m, 69, "intermittent"))
    none = aa.bit_autocorrelation(tc.pack(m), 70, matrix=False)
    assert "autocorrelation" not in none and np.array_equal(none["half_life"], full["half_life"])


def test_continuous_ends_at_the_longest_run():
    m = np.concatenate([ac.pattern("random0.5", 20, 200, seed=2), ac.pattern("random0.99", 5, 200, seed=3), ac.touching_runs().repeat(2, 1)[:, :200]])
    got = check_host(m, 199)
    stats = aa.timeline_stats(tc.pack(m), 200)
    cont = got["continuous"]["autocorrelation"]
    for r, longest in enumerate(stats["longest_run"].tolist()):
        assert not cont[r, longest:].any() and (longest == 0 or cont[r, longest - 1] > 0)
    assert np.array_equal(cont[:, 0], stats["n_present"])


def test_staircase_touching_runs_and_half_life_edges():
    ac.check_bitmap_reach()
    st = ac.staircase(70, 140)
    got = check_host(st, 69)
    assert np.array_equal(got["continuous"]["autocorrelation"], np.maximum(0, np.arange(70)[:, None] - np.arange(70)[None, :]))
    check_host(ac.touching_runs(), 99)
    m, F, t = ac.half_life_on_equality()
    got = check_host(m, F - 1)
    assert got["intermittent"]["half_life"][0] == t and got["intermittent"]["half_life"][2] == t and got["intermittent"]["half_life"][1] != t
    check_host(ac.late_half_life(), 399)


def test_bits_past_the_end_are_ignored():
    for rows, F in ((1, 1), (5, 40), (33, 65), (2, 1023)):
        m = sc.pattern("random0.5", rows, F, seed=3)
        words = sc.dirty(tc.pack(m), F)
        assert not np.array_equal(words, tc.pack(m))
        check_host(m, F - 1, ("dirty", rows, F), words=words)


def test_groups():
    m = ac.pattern("random0.5", 100, 65, seed=9)
    g = ac.groups_of(100)
    got = check_host(m, 64, "groups", group=g, n_groups=ac.N_GROUPS)
    for mode in ac.MODES:
        assert not got[mode]["sums"][[3, 7, 18]].any() and got[mode]["sums"][0].any()
        assert got[mode]["sums"].sum(0).tolist() == got[mode]["autocorrelation"].astype(np.uint64).sum(0).tolist()
    one = check_host(m, 64, "one group", group=np.full(100, 5, "<u4"), n_groups=7)
    assert one["intermittent"]["sums"][5].tolist() == one["intermittent"]["autocorrelation"].astype(np.uint64).sum(0).tolist()
    assert "sums" not in aa.bit_autocorrelation(tc.pack(m), 65)


def test_no_rows():
    got = aa.bit_autocorrelation(np.zeros((0, 2), "<u4"), 40, 10, group=np.zeros(0, "<u4"), n_groups=3)
    assert got["autocorrelation"].shape == (0, 11) and got["half_life"].shape == (0,) and got["sums"].shape == (3, 11) and not got["sums"].any()


def test_bad_arguments():
    words = np.zeros((2, 2), "<u4")
    acf, half, group, sums = np.zeros((2, 40), "<u4"), np.zeros(2, "<u4"), np.zeros(2, "<u4"), np.zeros((3, 40), "<u8")
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    q = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    host = lambda *a: aa.api._check(lib.arp_bit_autocorr_host(*a))
    refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, None, 0, 39, None, 0, p(acf), None, p(half), match="null")
    refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, p(words), 0, 39, None, 0, p(acf), None, None, match="null")
    refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, p(words), 0, 39, p(group), 3, p(acf), None, p(half), match="null")
    for flags in (0x1, 0x2, 0x20, 0x80000000):
        refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, p(words), flags, 39, None, 0, p(acf), None, p(half), match="unknown flag bits")
    for L in (40, 41, 0xFFFFFFFE):
        refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, p(words), 0, L, None, 0, p(acf), None, p(half), match="max_lag")
    group[1] = 3
    refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 40, p(words), 0, 39, p(group), 3, p(acf), q(sums), p(half), match="group[1] = 3")
    refused(_lib.ARP_ERR_BAD_INPUT, host, 2, 1 << 32, p(words), 0, 39, None, 0, p(acf), None, p(half), match="2^32")
    refused(_lib.ARP_ERR_BAD_INPUT, host, 1 << 32, 40, p(words), 0, 39, None, 0, p(acf), None, p(half), match="2^32")
    refused(_lib.ARP_ERR_BAD_INPUT, lambda: aa.api._check(lib.arp_bit_autocorr(None, 2, 40, p(words), 0, 39, None, 0, p(acf), None, p(half))), match="null")
    assert lib.arp_bit_autocorr_host(2, 40, p(words), 0, 39, None, 0, None, None, p(half)) == _lib.ARP_OK  # acf is nullable
    with pytest.raises(ValueError):
        aa.bit_autocorrelation(words, 65)
    with pytest.raises(ValueError):
        aa.bit_autocorrelation(words, 40, mode="survival")
    with pytest.raises(ValueError):
        aa.bit_autocorrelation(words, 40, group=np.zeros(3, "<u4"), n_groups=1)
    with pytest.raises(ValueError):
        aa.bit_autocorrelation(words, 40, max_lag=-1)


# ---- what arp_contact_autocorrelation decides before the device is touched ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


def frames_of(s: aa.Structure, F: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)[None].repeat(F, 0)


def checked(s, frames, groups="/", flags=0, level=0, max_lag=_lib.ARP_NONE) -> int:
    """arp_contact_autocorrelation with ctx == NULL: only the checks run."""
    n_frames, ptr, keep = aa.api._frames_arg(s, frames, "contact autocorrelation")
    t = C.c_void_p(1)
    st = lib.arp_contact_autocorrelation(None, s._h, int(n_frames), ptr, groups.encode(), 0.1, 6.5, flags, level, max_lag, C.byref(t))
    if st == _lib.ARP_OK:
        assert t.value is None  # *out = NULL
    return st


def test_null_context_runs_only_the_checks(ubq):
    for flags in (0, 0x1, 0x10, 0x20, 0x31):
        for level in (0, 1):
            for max_lag in (_lib.ARP_NONE, 0, 1):
                assert checked(ubq, frames_of(ubq, 2), flags=flags, level=level, max_lag=max_lag) == _lib.ARP_OK


@pytest.mark.parametrize("level", [-1, 2, 7])
def test_bad_level(ubq, level):
    assert checked(ubq, frames_of(ubq, 1), level=level) == _lib.ARP_ERR_BAD_INPUT
    assert "level" in lib.arp_last_error().decode()
    with pytest.raises(ValueError):
        aa.get_contact_autocorrelation(ubq, frames_of(ubq, 1), level="chain")
    with pytest.raises(ValueError):
        aa.get_contact_autocorrelation(ubq, frames_of(ubq, 1), mode="survival")


@pytest.mark.parametrize("flags", [_lib.ARP_TIMELINE_NO_BITMAP, _lib.ARP_SIM_COUNTS, _lib.ARP_SIM_ROWS, 0x40, 0x80000000, 0x3F])
def test_unknown_flag(ubq, flags):
    assert checked(ubq, frames_of(ubq, 1), flags=flags) == _lib.ARP_ERR_BAD_INPUT
    assert "unknown flag bits" in lib.arp_last_error().decode()


def test_max_lag_and_frame_limit(ubq):
    for max_lag in (3, 4, 1000):
        assert checked(ubq, frames_of(ubq, 3), max_lag=max_lag) == _lib.ARP_ERR_BAD_INPUT
        assert "max_lag" in lib.arp_last_error().decode()
    assert checked(ubq, frames_of(ubq, 3), max_lag=2) == _lib.ARP_OK
    # F > 2^24: a one-atom topology, so that the frames stay small
    import freq_edge_cases as fe

    top = fe.topology(["CC"], "AB")
    s = aa.Structure.from_records({k: v[:1] for k, v in top.rec.items()})
    assert s.n_atoms == 1
    F = (1 << 24) + 1
    xyz = np.zeros((F, 1, 3))
    assert checked(s, xyz) == _lib.ARP_ERR_BAD_INPUT
    msg = lib.arp_last_error().decode()
    assert f"F = {F}" in msg and "2^24" in msg
    assert checked(s, xyz[:1 << 24]) == _lib.ARP_OK


@pytest.mark.parametrize("level", ["atom", "residue"])
def test_input_errors_are_those_of_the_frequency_call(ubq, level, tmp_path, ubq_path):
    """Every error of the frequency call, with its status and message, whatever the device (the refusals of the timeline host test)."""
    import synth

    def same(*args, **kw):
        out = []
        for fn in (aa.get_contact_frequencies, aa.get_contact_autocorrelation):
            with pytest.raises(aa.ArpeggiaError) as e:
                fn(*args, level=level, **kw)
            out.append((e.value.status, str(e.value)))
        assert out[0] == out[1] or (out[0][0] == out[1][0] and out[0][1].replace("contact frequencies", "contact autocorrelation") == out[1][1]), out
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
    rec = synth.read_pdb_records(ubq_path)
    parts = []
    for m in range(3):
        r = {k: v.copy() for k, v in rec.items()}
        r["model_serial"][:] = m + 1
        parts.append(r)
    multi = {k: np.concatenate([p[k] for p in parts]) for k in rec}
    multi["name"][2 * len(rec["x"]) + 5] = b"CX"
    path = tmp_path / "differ.pdb"
    synth.write_pdb(multi, path)
    assert "model 2 (MODEL 3)" in same(aa.load_model(str(path)), None)
    refused(_lib.ARP_ERR_BAD_INPUT, aa.contact_autocorrelation, str(path), level=level, match="model 2 (MODEL 3)")


def test_cap_knob():
    aa.debug_set("autocorr_cap_bytes", 1)
    aa.debug_set("autocorr_cap_bytes", 1 << 40)
    aa.debug_set("autocorr_cap_bytes", 0)
    refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "autocorr_cap_bytes", -1)
    assert "autocorr_cap_bytes" in refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "no_such_knob", 1)


def test_table_autocorrelation_of_nothing():
    assert lib.arp_table_autocorrelation(None, None, None, None, None) is None


def test_cli_defaults_and_flags(tmp_path):
    from arpeggia_amd.__main__ import build_parser, main

    a = build_parser().parse_args(["contact-autocorrelation", "-i", "x.pdb", "-o", str(tmp_path)])
    assert (a.groups, a.filename, a.output_format, a.vdw_comp, a.dist_cutoff, a.num_threads, a.ignore_zero_occupancy, a.rings, a.level, a.mode, a.max_lag, a.matrix, a.curves) == \
        ("/", "contact_autocorrelation", "csv", 0.1, 6.5, 1, False, False, "atom", "intermittent", None, None, None)
    assert not hasattr(a, "bitmap")
    a = build_parser().parse_args(["contact-autocorrelation", "-i", "x.pdb", "-o", "d", "-g", "A/B", "-f", "f", "-t", "PARQUET", "-c", "0.2", "-d", "5", "-j", "4",
                                   "--ignore-zero-occupancy", "--rings", "-l", "residue", "--mode", "continuous", "--max-lag", "12", "--matrix", "m.npy", "--curves", "c.csv"])
    assert (a.groups, a.filename, a.output_format, a.vdw_comp, a.dist_cutoff, a.num_threads, a.ignore_zero_occupancy, a.rings, a.level, a.mode, a.max_lag, str(a.matrix),
            str(a.curves)) == ("A/B", "f", "parquet", 0.2, 5.0, 4, True, True, "residue", "continuous", 12, "m.npy", "c.csv")
    for bad in (["--mode", "survival"], ["--max-lag", "x"], ["--bitmap", "b.npy"], ["--axis", "rows"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["contact-autocorrelation", "-i", "x.pdb", "-o", "d"] + bad)
    assert main(["contact-autocorrelation", "-i", str(tmp_path / "none.pdb"), "-o", str(tmp_path)]) == 1
