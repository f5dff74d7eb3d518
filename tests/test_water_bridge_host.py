"""Water bridges on the CPU: the restatement of the definition (tests/water_bridge_restatement.py) equals the closed form of every built case
(tests/water_bridge_cases.py), every case reaches the edge it is named for, and the surface -- the checks that run without a device, the flag's
value, exports and header, the name of code 19, the Python signatures.  tests/test_water_bridge_gpu.py runs the cases on the device."""
from __future__ import annotations

import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import freq_residue_common as fc
import water_bridge_cases as wc
import water_bridge_restatement as wr
from arpeggia_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(wc.cases())
WATERS = 0x100
UBQ_COUNTS = (21, 20, 4)  # 1ubq as one frame: triples, residue rows, most partners of one water


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_closed_form(name):
    wc.check_reach(name)
    c = wc.cases()[name]
    s = aa.Structure.from_records(c.rec)
    assert s.n_atoms == c.n
    stats = {}
    got = wr.triples(s, c.frames, c.groups, stats)
    if c.capacity:
        assert stats["max_partners"] == wc.PARTNERS + 1
        return
    assert stats["max_partners"] <= wc.PARTNERS
    want = wc.expected_triples(c)
    for k in ("frame", "p", "q", "w"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("dp", "dq"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(s.soa("/")["res_id"][: c.n], c.res_of)  # the residue ordinals the closed form is written in
    fc.assert_same_table(wr.residue_rows(s, c.frames, c.groups), wc.expected_rows(c))
    pres, want_pres = wr.presence(s, c.frames, c.groups), wc.expected_presence(c)
    assert set(pres) == set(want_pres) and all(np.array_equal(pres[k], want_pres[k]) for k in pres)


def checked(fn, s: aa.Structure, *tail):
    """The call with ctx NULL and the structure's models as frames: (status, message)."""
    t = C.c_void_p()
    st = fn(None, s._h, 0, None, b"/", *tail, C.byref(t))
    assert not t.value
    return int(st), _lib.lib.arp_last_error().decode()


def test_flag_checks_without_a_device(ubq_path):
    lib = _lib.lib
    s = aa.load_model(ubq_path)
    assert _lib.ARP_FREQ_WATERS == WATERS
    # the residue frequency call takes the flag, alone or with the rings; the atom-level call never does
    assert checked(lib.arp_residue_contact_frequencies, s, 0.1, 6.5, WATERS)[0] == _lib.ARP_OK
    assert checked(lib.arp_residue_contact_frequencies, s, 0.1, 6.5, WATERS | _lib.ARP_FREQ_RINGS)[0] == _lib.ARP_OK
    st, msg = checked(lib.arp_contact_frequencies_ex, s, 0.1, 6.5, WATERS)
    assert st == _lib.ARP_ERR_BAD_INPUT and "unknown flag bits 0x100" in msg
    # timelines: level 1 takes it, level 0 names level 1 and arp_water_bridges
    for extra in (0, _lib.ARP_FREQ_RINGS, _lib.ARP_TIMELINE_NO_BITMAP):
        assert checked(lib.arp_contact_timelines, s, 0.1, 6.5, WATERS | extra, 1)[0] == _lib.ARP_OK
    st, msg = checked(lib.arp_contact_timelines, s, 0.1, 6.5, WATERS, 0)
    assert st == _lib.ARP_ERR_BAD_INPUT and "level 1" in msg and "arp_water_bridges" in msg
    # similarity, autocorrelation and clusters keep rejecting the bit as unknown, at either level
    for level in (0, 1):
        for fn, tail in ((lib.arp_contact_similarity, (level,)), (lib.arp_contact_autocorrelation, (level, _lib.ARP_NONE)), (lib.arp_contact_clusters, (level, 0.5, _lib.ARP_NONE))):
            st, msg = checked(fn, s, 0.1, 6.5, WATERS, *tail)
            assert st == _lib.ARP_ERR_BAD_INPUT and "unknown flag bits 0x100" in msg, (fn, level)
            assert checked(fn, s, 0.1, 6.5, 0, *tail)[0] == _lib.ARP_OK
    # arp_water_bridges: the frequency calls' checks
    assert checked(lib.arp_water_bridges, s)[0] == _lib.ARP_OK
    t = C.c_void_p()
    statuses = set()
    for groups in (b"", b"A", b"A/B/C,", b"Z/", b"/A", b"/"):  # the groups of test_freq_rings_host.py::test_checks_without_a_device
        want, want_msg = lib.arp_contact_frequencies_ex(None, s._h, 0, None, groups, 0.1, 6.5, 0, C.byref(t)), lib.arp_last_error()
        got, got_msg = lib.arp_water_bridges(None, s._h, 0, None, groups, C.byref(t)), lib.arp_last_error()
        assert got == want and (want == _lib.ARP_OK or got_msg == want_msg), groups
        statuses.add(want)
    assert statuses & {_lib.ARP_ERR_BAD_GROUPS, _lib.ARP_ERR_EMPTY_GROUPS} and _lib.ARP_OK in statuses
    xyz = np.zeros((2, s.n_atoms, 3))
    xyz[1, 5, 2] = np.inf
    ptr = xyz.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.arp_water_bridges(None, s._h, 0, ptr, b"/", C.byref(t)) == _lib.ARP_ERR_BAD_INPUT and b"at least one frame" in lib.arp_last_error()
    assert lib.arp_water_bridges(None, s._h, 2, ptr, b"/", C.byref(t)) == _lib.ARP_ERR_BAD_INPUT and b"frame 1, atom 5" in lib.arp_last_error()
    assert lib.arp_water_bridges(None, None, 1, ptr, b"/", C.byref(t)) == _lib.ARP_ERR_BAD_INPUT
    assert lib.arp_water_bridges(None, s._h, 1, ptr, b"/", None) == _lib.ARP_ERR_BAD_INPUT


def test_flag_values_are_distinct_powers_of_two():
    header = (ROOT / "include" / "arpeggia_amd.h").read_text()
    names = ("ARP_FREQ_RINGS", "ARP_TIMELINE_NO_BITMAP", "ARP_SIM_COUNTS", "ARP_SIM_ROWS", "ARP_ACF_CONTINUOUS", "ARP_ACF_NO_MATRIX", "ARP_CLUSTER_NO_COUNTS", "ARP_FREQ_WATERS")
    values = []
    for n in names:
        m = re.search(rf"^#define {n} (0x[0-9a-fA-F]+)u$", header, re.M)
        assert m, n
        assert int(m.group(1), 16) == getattr(_lib, n), n
        values.append(int(m.group(1), 16))
    assert all(v and v & (v - 1) == 0 for v in values) and len(set(values)) == len(names)
    assert _lib.ARP_FREQ_WATERS == 0x100 and 0x80 not in values


def test_exports_header_and_code_19():
    header = (ROOT / "include" / "arpeggia_amd.h").read_text()
    declared = sorted(set(re.findall(r"\b(arp_[a-z_0-9]+)\s*\(", header)))
    assert sorted(_lib.EXPORTS) == declared and "arp_water_bridges" in declared
    assert "arp_status arp_water_bridges(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, arp_table **out);" in header
    assert "#define ARP_WaterBridge 19" in header and "#define ARP_FREQ_WATERS 0x100u" in header
    for words in ("dx*dx + dy*dy + dz*dz <= 12.25", "the longer leg", "more than 32 polar atoms", "ARP_ERR_CAPACITY"):
        assert words in header, words
    lib = _lib.lib
    assert lib.arp_api_version() == 2
    assert lib.arp_interaction_name(19) == b"WaterBridge" and lib.arp_interaction_name(20) == b"?" and lib.arp_interaction_name(-1) == b"?"
    assert len(_lib.INTERACTIONS) == 19 and _lib.WATER_BRIDGE == 19 and _lib.ROW_CODES == _lib.INTERACTIONS + ["WaterBridge"]
    assert [lib.arp_interaction_name(k).decode() for k in range(20)] == _lib.ROW_CODES


def test_python_surface(ubq_path):
    for f in (aa.get_contact_frequencies, aa.contact_frequencies, aa.Context.contact_frequencies, aa.get_contact_timelines, aa.contact_timelines,
              aa.Context.contact_timelines):
        assert inspect.signature(f).parameters["waters"].default is False, f
    assert list(inspect.signature(aa.get_water_bridges).parameters) == ["structure", "frames", "groups", "device"]
    assert list(inspect.signature(aa.water_bridges).parameters) == ["input_file", "groups", "ignore_zero_occupancy"]
    assert hasattr(aa.Context, "water_bridges")
    names = [c for c, _ in aa.WATER_BRIDGE_COLUMNS]
    assert names[0] == "frame" and names[-3:] == ["from_distance", "to_distance", "distance"] and len(names) == 1 + 7 + 7 + 5 + 3
    assert [n for n in names if n.startswith("water_")] == ["water_chain", "water_resi", "water_insertion", "water_altloc", "water_atomi"]
    # level "atom" with waters: a ValueError before any device work (no context is ever made)
    s = aa.load_model(ubq_path)
    for call in (lambda: aa.get_contact_frequencies(s, waters=True), lambda: aa.get_contact_frequencies(s, waters=True, level="atom"),
                 lambda: aa.contact_frequencies(ubq_path, waters=True), lambda: aa.get_contact_timelines(s, waters=True, level="atom"),
                 lambda: aa.contact_timelines(ubq_path, waters=True), lambda: aa.api._freq_table(None, s, None, "/", 0.1, 6.5, False, "atom", True),
                 lambda: aa.api._timeline_table(None, s, None, "/", 0.1, 6.5, False, "atom", True, True)):
        with pytest.raises(ValueError, match="level='residue'"):
            call()
    # with level "residue" the checks pass without a device
    assert aa.api._freq_table(None, s, None, "/", 0.1, 6.5, False, "residue", True) is None
    assert aa.api._timeline_table(None, s, None, "/", 0.1, 6.5, True, "residue", True, True) is None
    assert aa.api._water_bridge_table(None, s, None, "/") is None


def test_cli_needs_the_residue_level(ubq_path, tmp_path):
    from arpeggia_amd.__main__ import build_parser, main

    args = build_parser().parse_args(["water-bridges", "-i", ubq_path, "-o", str(tmp_path), "-g", "/", "-t", "csv"])
    assert args.command == "water-bridges" and args.filename == "water_bridges"
    for cmd in ("contact-frequency", "contact-timeline"):
        assert build_parser().parse_args([cmd, "-i", ubq_path, "-o", str(tmp_path), "-l", "residue", "--waters"]).waters
        assert main([cmd, "-i", ubq_path, "-o", str(tmp_path / "out"), "--waters"]) == 1  # (atom level)
    assert not (tmp_path / "out").exists()


def test_ubq_restatement_counts(ubq_path):
    """1ubq as one frame: the numbers DESIGN.md section 3.19 records."""
    s = aa.load_model(ubq_path)
    n = s.n_atoms
    soa = s.soa("/")
    xyz = np.stack([soa["x"], soa["y"], soa["z"]], axis=1)[None]
    stats = {}
    t = wr.triples(s, xyz, "/", stats)
    rows = wr.residue_rows(s, xyz, "/")
    assert stats["n_water"] == 58 and n == 660
    assert (len(t), len(rows["n_frames"]), stats["max_partners"]) == UBQ_COUNTS
