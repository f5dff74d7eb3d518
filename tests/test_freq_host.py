"""Contact frequencies across frames: everything that is decided before the device is touched (CLI, knob, input checks)."""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import synth
from arpeggia_amd import _lib


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


def frames_of(s: aa.Structure, F: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)[None].repeat(F, 0)


def refused(status: int, fn, *args, match: str | None = None):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args)
    assert e.value.status == status, str(e.value)
    if match:
        assert match in str(e.value)
    return str(e.value)


def test_cli_defaults_and_flags(tmp_path):
    from arpeggia_amd.__main__ import build_parser

    a = build_parser().parse_args(["contact-frequency", "-i", "x.pdb", "-o", str(tmp_path)])
    assert (a.groups, a.filename, a.output_format, a.vdw_comp, a.dist_cutoff, a.num_threads, a.ignore_zero_occupancy) == \
        ("/", "contact_frequency", "csv", 0.1, 6.5, 1, False)
    a = build_parser().parse_args(["contact-frequency", "-i", "x.pdb", "-o", "d", "-g", "A/B", "-f", "f", "-t", "PARQUET", "-c", "0.2", "-d", "5",
                                   "-j", "4", "--ignore-zero-occupancy"])
    assert (a.groups, a.filename, a.output_format, a.vdw_comp, a.dist_cutoff, a.num_threads, a.ignore_zero_occupancy) == \
        ("A/B", "f", "parquet", 0.2, 5.0, 4, True)


def test_cli_missing_input(tmp_path):
    from arpeggia_amd.__main__ import main

    assert main(["contact-frequency", "-i", str(tmp_path / "none.pdb"), "-o", str(tmp_path)]) == 1


def test_chunk_knob():
    aa.debug_set("freq_chunk_atoms", 1000)
    aa.debug_set("freq_chunk_atoms", 0)
    refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "freq_chunk_atoms", -1)


def test_cap_knob():
    aa.debug_set("freq_cap_items", 1)
    aa.debug_set("freq_cap_items", 0)
    refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "freq_cap_items", -1)
    assert "freq_cap_items" in refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "no_such_knob", 1)


def test_exported():
    assert "arp_contact_frequencies" in _lib.EXPORTS
    assert [c for c, _ in aa.FREQ_COLUMNS][-4:] == ["n_frames", "frequency", "min_distance", "max_distance"]


def test_zero_frames(ubq):
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_contact_frequencies, ubq, frames_of(ubq, 0), match="at least one frame")


@pytest.mark.parametrize("shape", [(2, 5, 3), (2, 660, 2), (660, 3), (1, 2, 660, 3)])
def test_wrong_shape(ubq, shape):
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_contact_frequencies, ubq, np.zeros(shape), match="shape")


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite(ubq, value):
    f = frames_of(ubq, 3)
    f[2, 17, 1] = value
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_contact_frequencies, ubq, f, match="frame 2, atom 17")


def _models(rec: dict, F: int) -> dict:
    parts = []
    for m in range(F):
        r = {k: v.copy() for k, v in rec.items()}
        r["model_serial"][:] = m + 1
        parts.append(r)
    return {k: np.concatenate([p[k] for p in parts]) for k in rec}


def test_models_that_differ(tmp_path, ubq_path):
    rec = synth.read_pdb_records(ubq_path)
    multi = _models(rec, 3)
    n = len(rec["x"])
    multi["name"][2 * n + 5] = b"CX"  # model 2 (MODEL 3), atom 5
    path = tmp_path / "differ.pdb"
    synth.write_pdb(multi, path)
    s = aa.load_model(str(path))
    msg = refused(_lib.ARP_ERR_BAD_INPUT, aa.get_contact_frequencies, s, None, match="model 2 (MODEL 3)")
    assert "atom 5" in msg and "atom name" in msg
    refused(_lib.ARP_ERR_BAD_INPUT, aa.contact_frequencies, str(path), match="model 2 (MODEL 3)")


def test_models_with_different_atom_counts(tmp_path, ubq_path):
    rec = synth.read_pdb_records(ubq_path)
    multi = _models(rec, 2)
    keep = np.ones(len(multi["x"]), bool)
    keep[-3] = False  # model 1 loses an atom near its end
    path = tmp_path / "short.pdb"
    synth.write_pdb({k: v[keep] for k, v in multi.items()}, path)
    s = aa.load_model(str(path))
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_contact_frequencies, s, None, match="model 1 (MODEL 2)")


@pytest.mark.parametrize("groups", ["", "A", "A/B/C,", "Z/", "/A"])
def test_group_errors_are_those_of_get_contacts(ubq, groups):
    from arpeggia_amd import api

    want = None
    try:
        api.parse_groups(["A"], groups)
    except aa.ArpeggiaError as e:
        want = (e.status, str(e))
    try:
        aa.get_contact_frequencies(ubq, frames_of(ubq, 1), groups)
        got = None
    except aa.ArpeggiaError as e:
        got = (e.status, str(e))
    if want is None:  # a valid spec: only the missing device (CPU machine) or nothing (GPU machine) may be reported
        assert got is None or got[0] == _lib.ARP_ERR_NO_DEVICE
    else:
        assert got == want
        assert want[0] in (_lib.ARP_ERR_BAD_GROUPS, _lib.ARP_ERR_EMPTY_GROUPS)
