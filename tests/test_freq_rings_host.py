"""Ring rows of contact frequencies across frames, on the CPU: the built cases of tests/freq_ring_cases.py against the oracle frame by frame, and
the surface of arp_contact_frequencies_ex (export, flags, the checks that run without a device, CLI and Python signatures)."""
from __future__ import annotations

import ctypes as C
import inspect
from pathlib import Path

import pytest

import arpeggia_amd as aa
import freq_ring_cases as rc
import oracle_binding as ob
import synth
from arpeggia_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
DIST_TOL = 1e-5  # the project's distance tolerance against the oracle (f32 table distances)


def oracle_ring_rows(case: rc.Case) -> dict:
    """identity + code -> [distances] over the frames: the rows with a Ring entity of one oracle get_contacts call per frame (single-model
    structures from the hierarchy builder, flat=False)."""
    out = {}
    for f in range(case.F):
        s = ob.Structure.from_atoms(synth.records_to_oracle(rc.frame_records(case, f), flat=False), flat=False)
        rows = s.get_contacts("/", 0.1, 6.5)
        ring = rows[(rows["from"]["atomn"] == b"Ring") | (rows["to"]["atomn"] == b"Ring")]
        for r in ring:
            assert r["from"]["atomn"] == b"Ring" and r["from"]["atomi"] == 0 and r["from_atom"] == -1
            key = (bytes(r["from"]["chain"]), int(r["from"]["resi"]), bytes(r["from"]["altloc"]), bytes(r["to"]["chain"]), int(r["to"]["resi"]),
                   bytes(r["to"]["atomn"]), int(r["interaction"]))
            out.setdefault(key, []).append(float(r["distance"]))
    return out


@pytest.mark.parametrize("case", rc.all_cases(), ids=lambda c: c.name)
def test_closed_form_is_the_oracle(case):
    want = rc.expected(case)
    got = oracle_ring_rows(case)
    keys = [(bytes(want["from_chain"][k]), int(want["from_resi"][k]), bytes(want["from_altloc"][k]), bytes(want["to_chain"][k]), int(want["to_resi"][k]),
             bytes(want["to_atomn"][k]), int(want["interaction"][k])) for k in range(len(want["interaction"]))]
    assert len(set(keys)) == len(keys) > 0
    assert set(keys) == set(got)
    for k, key in enumerate(keys):
        d = got[key]
        assert len(d) == want["n_frames"][k], key
        assert abs(min(d) - want["min_distance"][k]) <= DIST_TOL and abs(max(d) - want["max_distance"][k]) <= DIST_TOL, key
    # every branch of the ladder and the cation rule is there, and the altloc motif gives its rows twice
    assert set(want["interaction"].tolist()) == set(rc.CODES.values())
    assert (want["from_altloc"] == b"A").sum() == (want["from_altloc"] == b"B").sum() > 0


@pytest.mark.parametrize("case", rc.all_cases(), ids=lambda c: c.name)
def test_cases_reach_their_edges(case):
    one, three = rc.edges(case, case.F), rc.edges(case, case.per_for_passes(3))
    assert {"fit64", "fit128", "fit256", "items64", "items256"} <= one
    assert {"fit64", "fit128", "fit256", "items64", "partial"} <= three
    if case.name == "small":
        assert "keybit" in one & three
    if case.name == "wide":
        assert {"tile2", "ring64", "ring256", "cand64", "cand256"} <= one & three
    assert rc.min_distance_between_residues(case) > 1.0  # (dist_cutoff = 1.0 leaves no atom row)


def test_entry_point_is_exported_and_declared():
    assert hasattr(_lib.lib, "arp_contact_frequencies_ex")
    assert _lib.ARP_FREQ_RINGS == 0x1
    header = (ROOT / "include" / "arpeggia_amd.h").read_text()
    assert "#define ARP_FREQ_RINGS 0x1u" in header
    assert "arp_status arp_contact_frequencies_ex(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,\n" \
           "                                      double dist_cutoff, uint32_t flags, arp_table **out);" in header
    assert _lib.lib.arp_api_version() == 2


def call_ex(s: aa.Structure, groups: str, flags: int) -> int:
    t = C.c_void_p()
    st = _lib.lib.arp_contact_frequencies_ex(None, s._h, 0, None, groups.encode(), 0.1, 6.5, flags, C.byref(t))
    assert not t.value
    return int(st)


def test_checks_without_a_device(ubq_path):
    s = aa.load_model(ubq_path)
    assert call_ex(s, "/", 0) == _lib.ARP_OK
    assert call_ex(s, "/", _lib.ARP_FREQ_RINGS) == _lib.ARP_OK
    for bad in (0x2, 0x3, 0x80000000):
        assert call_ex(s, "/", bad) == _lib.ARP_ERR_BAD_INPUT
        assert b"flag" in _lib.lib.arp_last_error()
    statuses = set()
    for groups in ("", "A", "A/B/C,", "Z/", "/A", "/"):
        t = C.c_void_p()
        old = int(_lib.lib.arp_contact_frequencies(None, s._h, 0, None, groups.encode(), 0.1, 6.5, C.byref(t)))
        old_msg = _lib.lib.arp_last_error()
        for flags in (0, _lib.ARP_FREQ_RINGS):
            assert call_ex(s, groups, flags) == old
            if old != _lib.ARP_OK:
                assert _lib.lib.arp_last_error() == old_msg
        statuses.add(old)
    assert statuses & {_lib.ARP_ERR_BAD_GROUPS, _lib.ARP_ERR_EMPTY_GROUPS} and _lib.ARP_OK in statuses


def test_a_topology_without_rings_passes_the_checks():
    import freq_edge_cases as ec

    s = aa.Structure.from_records(ec.topology(["CC", "ON"]).rec)
    assert call_ex(s, "/", _lib.ARP_FREQ_RINGS) == _lib.ARP_OK


def test_cli_and_python_signatures():
    from arpeggia_amd.__main__ import build_parser

    args = build_parser().parse_args(["contact-frequency", "-i", "x.pdb", "-o", "out"])
    assert args.rings is False
    assert build_parser().parse_args(["contact-frequency", "-i", "x.pdb", "-o", "out", "--rings"]).rings is True
    for fn in (aa.Context.contact_frequencies, aa.get_contact_frequencies, aa.contact_frequencies):
        p = inspect.signature(fn).parameters
        assert "rings" in p and p["rings"].default is False, fn
