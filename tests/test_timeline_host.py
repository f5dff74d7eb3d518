"""Contact timelines across frames: everything that needs no device.  arp_timeline_stats (the sequential restatement of the definition, and the CPU
yardstick of k_timeline_stats) against a brute-force Python loop; the closed-form timelines of tests/timeline_cases.py against the oracle, one
atomic_contacts call per frame; every case's reach assertions; the checks arp_contact_timelines runs before the device is touched; the CLI's
flags; unpack_timeline."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import arpeggia_amd as aa
import freq_edge_cases as fe
import timeline_cases as tc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib

NAMES = list(tc.cases())


def refused(status: int, fn, *args, match: str | None = None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    if match:
        assert match in str(e.value)
    return str(e.value)


def check_stats(masks: np.ndarray):
    masks = np.asarray(masks, bool)
    got = aa.timeline_stats(tc.pack(masks), masks.shape[1])
    want = [tc.brute(m) for m in masks]
    for k, name in enumerate(("n_present", "first_frame", "last_frame", "n_events", "longest_run")):
        assert got[name].dtype == np.dtype("<u4")
        assert got[name].tolist() == [w[k] for w in want], name


def test_exported():
    for name in ("arp_contact_timelines", "arp_table_timeline", "arp_timeline_stats"):
        assert name in _lib.EXPORTS
    assert [c for c, _ in aa.TIMELINE_COLUMNS] == tc.STAT_COLUMNS
    assert lib.arp_api_version() == 2  # additive exports do not move the layout version


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_boundary(name):
    tc.check_reach(name)


@pytest.mark.parametrize("name", NAMES)
def test_stats_of_the_cases(name):
    """arp_timeline_stats == the brute-force loop on every case's bitmap; the packed words of the closed form unpack to the masks."""
    c = tc.cases()[name]
    _, masks = tc.row_masks(c.top, c.D)
    check_stats(masks)
    want = tc.expected_of(name)
    assert np.array_equal(aa.unpack_timeline(want["timeline_words"], c.F), masks)
    got = aa.timeline_stats(want["timeline_words"], c.F)
    assert np.array_equal(got["n_present"], want["n_frames"])
    for a, b in (("first_frame", "first_frame"), ("last_frame", "last_frame"), ("n_events", "n_events"), ("longest_run", "longest_run")):
        assert np.array_equal(got[a], want[b]), a


@pytest.mark.parametrize("F", [1, 2, 31, 32, 33, 64, 65, 95, 96, 2047, 2048, 2049, 4097])
def test_stats_patterns(F):
    """All set, none set, alternating from 0 and from 1, only frame 0, only frame F - 1, everything but one frame, and runs up to word edges."""
    f = np.arange(F)
    rows = [np.ones(F, bool), np.zeros(F, bool), f % 2 == 0, f % 2 == 1, f == 0, f == F - 1, f != F // 2, f < 32, f >= F - min(F, 33), (f >= 31) & (f <= 64),
            (f // 32) % 2 == 0, (f % 32 != 31), (f % 32 != 0)]
    check_stats(np.stack(rows))
    none = aa.timeline_stats(tc.pack(np.zeros((1, F), bool)), F)
    assert (none["first_frame"][0], none["last_frame"][0], none["n_events"][0], none["longest_run"][0], none["n_present"][0]) == (tc.NONE, tc.NONE, 0, 0, 0)


@pytest.mark.parametrize("seed,F,density", [(0, 1, 0.5), (1, 37, 0.5), (2, 64, 0.9), (3, 200, 0.1), (4, 2050, 0.97), (5, 2050, 0.5), (6, 4100, 0.999)])
def test_stats_random(seed, F, density):
    check_stats(np.random.default_rng(seed).random((23, F)) < density)


def test_stats_ignore_bits_past_the_last_frame():
    """Set bits past n_frames in the last word are not counted (the table's own bitmaps have none)."""
    words = np.array([[0xFFFFFFFF, 0xFFFFFFFF]], "<u4")
    got = aa.timeline_stats(words, 40)
    assert (got["n_present"][0], got["first_frame"][0], got["last_frame"][0], got["n_events"][0], got["longest_run"][0]) == (40, 0, 39, 1, 40)
    refused(_lib.ARP_ERR_BAD_INPUT, lambda: aa.api._check(lib.arp_timeline_stats(1, 40, None, None, None, None, None, None)), match="null")
    with pytest.raises(ValueError):
        aa.timeline_stats(words, 65)


def test_unpack_round_trip():
    rng = np.random.default_rng(7)
    for F in (1, 31, 32, 33, 100, 2049):
        masks = rng.random((5, F)) < 0.5
        words = tc.pack(masks)
        assert words.shape == (5, (F + 31) // 32)
        got = aa.unpack_timeline(words, F)
        assert got.dtype == bool and got.shape == (5, F) and np.array_equal(got, masks)
        assert np.array_equal(got, np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :F].astype(bool))
    assert aa.unpack_timeline(np.zeros((0, 2), "<u4"), 40).shape == (0, 40)
    with pytest.raises(ValueError):
        aa.unpack_timeline(np.zeros((2, 2), "<u4"), 100)


@pytest.mark.parametrize("name", ["run_boundaries", "passes_gap", "mark_mixed"])
def test_closed_form_equals_oracle(name):
    """The closed-form timeline against one oracle atomic_contacts call per frame (freq_edge_cases.oracle_table's loop, keeping the frames).
    run_boundaries: on the frames around every run end and boundary, not all 2100."""
    c = tc.cases()[name]
    if name == "run_boundaries":
        edges = {0, c.F - 1, 31, 32, 63, 64, 127, 128, 2047, 2048}
        for rr in tc.BOUNDARY_RUNS.values():
            edges |= {f for a, b in rr for f in (a - 1, a, b, b + 1)}
        sub = np.array(sorted(f for f in edges if 0 <= f < c.F))
        D = c.D[sub]
    else:
        D = c.D
    keys, masks = tc.row_masks(c.top, D)
    got = tc.oracle_masks(c.top, D)
    assert sorted(got) == [tuple(map(int, k)) for k in keys]
    for k, m in zip(keys, masks):
        assert np.array_equal(got[tuple(map(int, k))], m), k


# ---- what arp_contact_timelines decides before the device is touched -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


def frames_of(s: aa.Structure, F: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)[None].repeat(F, 0)


def checked(s, frames, groups="/", flags=0, level=0) -> int:
    """arp_contact_timelines with ctx == NULL: only the checks run."""
    n_frames, ptr, keep = aa.api._frames_arg(s, frames, "contact timelines")
    t = C.c_void_p(1)
    st = lib.arp_contact_timelines(None, s._h, int(n_frames), ptr, groups.encode(), 0.1, 6.5, flags, level, C.byref(t))
    if st == _lib.ARP_OK:
        assert t.value is None  # *out = NULL
    return st


def test_null_context_runs_only_the_checks(ubq):
    for flags in (0, _lib.ARP_FREQ_RINGS, _lib.ARP_TIMELINE_NO_BITMAP, _lib.ARP_FREQ_RINGS | _lib.ARP_TIMELINE_NO_BITMAP):
        for level in (0, 1):
            assert checked(ubq, frames_of(ubq, 2), flags=flags, level=level) == _lib.ARP_OK


@pytest.mark.parametrize("level", [-1, 2, 7])
def test_bad_level(ubq, level):
    assert checked(ubq, frames_of(ubq, 1), level=level) == _lib.ARP_ERR_BAD_INPUT
    assert "level" in lib.arp_last_error().decode()
    with pytest.raises(ValueError):
        aa.get_contact_timelines(ubq, frames_of(ubq, 1), level="chain")


@pytest.mark.parametrize("flags", [0x4, 0x8, 0x80000000, 0x7])
def test_unknown_flag(ubq, flags):
    assert checked(ubq, frames_of(ubq, 1), flags=flags) == _lib.ARP_ERR_BAD_INPUT
    assert "unknown flag bits" in lib.arp_last_error().decode()


@pytest.mark.parametrize("level", ["atom", "residue"])
def test_input_errors_are_those_of_the_frequency_call(ubq, level, tmp_path, ubq_path):
    """Every error of the frequency call, with its status and message, whatever the device."""
    import synth

    def same(*args, **kw):
        out = []
        for fn in (aa.get_contact_frequencies, aa.get_contact_timelines):
            with pytest.raises(aa.ArpeggiaError) as e:
                fn(*args, level=level, **kw)
            out.append((e.value.status, str(e.value)))
        assert out[0] == out[1] or (out[0][0] == out[1][0] and out[0][1].replace("contact frequencies", "contact timelines") == out[1][1]), out
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
    refused(_lib.ARP_ERR_BAD_INPUT, aa.contact_timelines, str(path), level=level, match="model 2 (MODEL 3)")


def test_cap_knob():
    aa.debug_set("timeline_cap_bytes", 1)
    aa.debug_set("timeline_cap_bytes", 1 << 40)
    aa.debug_set("timeline_cap_bytes", 0)
    refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "timeline_cap_bytes", -1)
    assert "timeline_cap_bytes" in refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "no_such_knob", 1)


def test_table_timeline_of_nothing():
    assert lib.arp_table_timeline(None, None, None) is None


def test_cli_defaults_and_flags(tmp_path):
    from arpeggia_amd.__main__ import build_parser, main

    a = build_parser().parse_args(["contact-timeline", "-i", "x.pdb", "-o", str(tmp_path)])
    assert (a.groups, a.filename, a.output_format, a.vdw_comp, a.dist_cutoff, a.num_threads, a.ignore_zero_occupancy, a.rings, a.level, a.bitmap) == \
        ("/", "contact_timeline", "csv", 0.1, 6.5, 1, False, False, "atom", None)
    a = build_parser().parse_args(["contact-timeline", "-i", "x.pdb", "-o", "d", "-g", "A/B", "-f", "f", "-t", "PARQUET", "-c", "0.2", "-d", "5", "-j", "4",
                                   "--ignore-zero-occupancy", "--rings", "-l", "residue", "--bitmap", "b.npy"])
    assert (a.groups, a.filename, a.output_format, a.vdw_comp, a.dist_cutoff, a.num_threads, a.ignore_zero_occupancy, a.rings, a.level, str(a.bitmap)) == \
        ("A/B", "f", "parquet", 0.2, 5.0, 4, True, True, "residue", "b.npy")
    assert main(["contact-timeline", "-i", str(tmp_path / "none.pdb"), "-o", str(tmp_path)]) == 1
