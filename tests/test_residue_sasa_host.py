"""CPU checks of the residue- / chain-level SASA surface: the radius tables, MaxASA, the reference's chain-level pin
restated with the ProtOr radii, the checks of arp_segment_sum and arp_sasa_ensemble_residues through a NULL context, and the CLI.  No compute
call is made."""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import ens_sasa_common as ec
import residue_sasa_common as rc
from arpeggia_amd import _lib
from arpeggia_amd.__main__ import build_parser, main
from arpeggia_amd.api import _residue_sasa_ensemble

ELEMENT_OF = {"C": "C", "N": "N", "O": "O", "S": "S"}


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.Structure.load(ubq_path)


def refused(fn, *args, match=None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == _lib.ARP_ERR_BAD_INPUT, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


# ---- 1. the radius tables ---------------------------------------------------------------------------------------------------------------------
def test_protor_radius_of_every_residue_atom_pair():
    n = 0
    for resn in rc.AMINO_ACIDS:
        for atomn in sorted({a for r, a in rc.PROTOR if r in (resn, "ANY")}):
            want, fell_back = rc.protor_radius(resn, atomn, ELEMENT_OF[atomn[0]])
            assert not fell_back
            got = aa.sasa_radius(resn, atomn, ELEMENT_OF[atomn[0]], "protor")
            assert np.float32(got) == np.float32(want), (resn, atomn, got, want)
            assert aa.sasa_radius(resn.lower(), atomn, ELEMENT_OF[atomn[0]], "protor") == got  # the residue name is matched case-insensitively
            n += 1
    assert n == sum(len({a for r, a in rc.PROTOR if r in (resn, "ANY")}) for resn in rc.AMINO_ACIDS) and n > 20 * 6  # (six ANY names per residue and the side chains)


def test_protor_specific_rows_win_over_any():
    assert np.float32(aa.sasa_radius("PRO", "N", "N")) == np.float32(1.64) and rc.PROTOR[("PRO", "N")] == rc.CLASSES["N3H0"]
    assert np.float32(aa.sasa_radius("GLY", "CA", "C")) == np.float32(1.88)
    assert np.float32(aa.sasa_radius("ASP", "CG", "C")) == np.float32(1.61)  # the side chain's C3H0, not a generic carbon
    assert np.float32(aa.sasa_radius("SER", "OG", "O")) == np.float32(1.46) and np.float32(aa.sasa_radius("SER", "O", "O")) == np.float32(1.42)
    assert np.float32(aa.sasa_radius("MSE", "CB", "C")) == np.float32(1.88)  # (ANY, CB) for a residue the table does not list


def test_vdw_table_is_the_element_radius():
    p = aa.default_params()
    for sym in ("C", "N", "O", "S", "P", "FE", "ZN", "SE"):
        c = _lib.lib.arp_element_class(sym.encode())
        if c < 0 or not p.vdw_radius[c] > 0:
            continue
        assert np.float32(aa.sasa_radius("ALA", "CB", sym, "vdw")) == np.float32(p.vdw_radius[c]), sym
        assert np.float32(aa.sasa_radius("HEM", "X1", sym, "protor")) == np.float32(p.vdw_radius[c]), sym  # an unknown atom name: the element's radius
    assert np.float32(aa.sasa_radius("ALA", "CB", "C", "vdw")) != np.float32(aa.sasa_radius("ALA", "CB", "C", "protor"))


def test_unknown_table_is_refused():
    with pytest.raises(ValueError):
        aa.sasa_radius("ALA", "CB", "C", "chothia")
    out = _lib.C.c_float()
    assert _lib.lib.arp_sasa_radius(b"ALA", b"CB", b"C", 2, _lib.C.byref(out)) == _lib.ARP_ERR_BAD_INPUT
    assert _lib.lib.arp_sasa_radius(b"ALA", b"CB", b"C", -1, _lib.C.byref(out)) == _lib.ARP_ERR_BAD_INPUT
    assert _lib.lib.arp_sasa_radius(b"HEM", b"X1", b"QQ", 1, _lib.C.byref(out)) == _lib.ARP_ERR_BAD_INPUT  # no row and no element radius
    for fn in (aa.get_atom_sasa, aa.get_residue_sasa, aa.get_chain_sasa, aa.get_relative_sasa):
        with pytest.raises(ValueError):
            fn(None, radii="chothia")  # (refused before the structure or the device is looked at)


# ---- 2. the reference's chain-level pin, restated on the CPU ----------------------------------------------------------------------------------
def test_1ubq_chain_total_with_protor_radii_is_the_reference_pin(ubq):
    """The reference's test_sasa_regression_ubiquitin: "around 4813" (+- 100 there); +- 1 here is the rounding of that number, not a tolerance
    on a kernel (the counts are integers).  Measured: 4813.18."""
    total = rc.protor_total_of_1ubq(ubq)
    print("1ubq chain total, ProtOr radii:", total)
    assert abs(total - 4813.0) <= 1.0
    # and the library's table gives the same radii as the helper's for these 602 atoms
    sel = rc.select_1_to_4(ubq)
    want, _ = rc.table_radii(ubq, sel, "protor")
    got = [aa.sasa_radius(r.decode(), a.decode(), e.decode()) for r, a, e in zip(ubq.strings("resn")[sel], ubq.strings("atomn")[sel], ubq.strings("element")[sel])]
    assert np.array_equal(np.array(got, np.float32), want)


# ---- 3. MaxASA and the polar list -------------------------------------------------------------------------------------------------------------
def test_max_asa_is_the_reference_table():
    assert len(rc.MAX_ASA) == 20
    for resn, v in rc.MAX_ASA.items():
        assert aa.max_asa(resn) == v and aa.max_asa(resn.lower()) == v
    for resn in ("XXX", "HOH", "", "ALAA"):
        assert aa.max_asa(resn) is None
    for resn in rc.AMINO_ACIDS + ["HOH", "XXX"]:
        assert _lib.lib.arp_residue_is_polar(resn.encode()) == int(resn in rc.POLAR)


# ---- 4. the checks of arp_segment_sum and arp_sasa_ensemble_residues (NULL context) --------------------------------------------------------------
def test_segment_sum_checks():
    v = np.ones((2, 5), np.float32)
    assert aa.segment_sum(None, v, [0, 2, 5], [0, 1, 2, 3, 4]).shape == (2, 2)
    assert aa.segment_sum(None, v, [0, 0, 0], []).shape == (2, 2)            # empty segments
    assert aa.segment_sum(None, v, [0, 3, 6], [4, 4, 0, 0, 4, 1]).shape == (2, 2)  # an item in two segments, any order
    refused(aa.segment_sum, None, v, [0, 2, 5], [0, 1, 2, 3, 5], match="not below m")
    refused(aa.segment_sum, None, v, [0, 3, 2], [0, 1, 2], match="monotone")
    refused(aa.segment_sum, None, v, [1, 2], [0, 1], match="seg_start[0]")
    # nothing to do is not an error, whatever the lists hold
    assert aa.segment_sum(None, np.zeros((0, 5), np.float32), [0, 1], [9]).shape == (0, 1)
    assert aa.segment_sum(None, np.zeros((3, 0), np.float32), [0, 1], [9]).shape == (3, 1)
    assert aa.segment_sum(None, v, [0], []).shape == (2, 0)


def test_residue_ensemble_checks(ubq):
    frames = ec.topology_xyz(ubq)[None].repeat(3, 0)
    r = _residue_sasa_ensemble(None, ubq, frames, "", 1.4, 100, "protor", False)
    assert r["n_frames"] == 3 and len(r["res_atoms"]) == 76 and len(r["chain_atoms"]) == 1
    assert [c.decode() for c in ubq.strings("chain")[r["chain_atoms"]]] == ["A"]
    assert ubq.ints("resi")[r["res_atoms"]].tolist() == list(range(1, 77))
    r = _residue_sasa_ensemble(None, ubq, frames, "Q", 1.4, 100, "vdw", False)
    assert r["n_frames"] == 3 and len(r["res_atoms"]) == 0 and len(r["chain_atoms"]) == 0
    refused(_residue_sasa_ensemble, None, ubq, frames[:0], "", 1.4, 100, "protor", False, match="at least one frame")
    refused(_residue_sasa_ensemble, None, ubq, frames, "", 1.4, 0, "protor", False, match="n_points must be 1..4096")
    refused(_residue_sasa_ensemble, None, ubq, frames, "", -1.0, 100, "protor", False, match="probe radius")
    refused(_residue_sasa_ensemble, None, ubq, np.zeros((2, 5, 3)), "", 1.4, 100, "protor", False, match="shape")
    bad = frames.copy()
    bad[2, 17, 1] = np.nan
    refused(_residue_sasa_ensemble, None, ubq, bad, "", 1.4, 100, "protor", False, match="frame 2, atom 17")
    refused(aa.get_residue_sasa_ensemble, ubq, bad, match="frame 2, atom 17")  # also ahead of a missing device
    with pytest.raises(ValueError):
        _residue_sasa_ensemble(None, ubq, frames, "", 1.4, 100, "chothia", False)
    rows, chains, used = _lib.C.c_uint64(), _lib.C.c_uint64(), _lib.C.c_uint64()
    st = _lib.lib.arp_sasa_ensemble_residues(None, ubq._h, 3, frames.ctypes.data_as(_lib._dp), b"", _lib.C.c_float(1.4), 100, 7, _lib.C.byref(rows),
                                             _lib.C.byref(chains), _lib.C.byref(used), *([None] * 11))
    assert st == _lib.ARP_ERR_BAD_INPUT and b"radius table" in _lib.lib.arp_last_error()


def test_exports_and_columns():
    new = {"arp_sasa_radius", "arp_max_asa", "arp_residue_is_polar", "arp_segment_sum", "arp_structure_residue_sasa", "arp_structure_chain_sasa",
           "arp_structure_relative_sasa", "arp_structure_atom_sasa_radii", "arp_structure_dsasa_radii", "arp_sasa_ensemble_radii", "arp_sasa_ensemble_residues"}
    assert new <= set(_lib.EXPORTS)
    assert _lib.lib.arp_api_version() == 2
    assert aa.RESIDUE_SASA_COLUMNS == ["chain", "resn", "resi", "insertion", "sasa", "is_polar"]
    assert aa.CHAIN_SASA_COLUMNS == ["chain", "sasa"]
    assert aa.RELATIVE_SASA_COLUMNS == aa.RESIDUE_SASA_COLUMNS + ["relative_sasa"]  # the reference's code: no altloc, no max_sasa
    for name in ("get_residue_sasa", "get_chain_sasa", "get_relative_sasa", "relative_sasa", "get_residue_sasa_ensemble", "segment_sum"):
        assert callable(getattr(aa, name))
    assert callable(aa.Context.residue_sasa_ensemble)


# ---- 5. the CLI -------------------------------------------------------------------------------------------------------------------------------
def test_cli_relative_sasa_carries_the_reference_defaults():
    ap = build_parser()
    a = ap.parse_args(["relative-sasa", "-i", "x.pdb", "-o", "out"])
    assert (a.filename, a.output_format, a.model_num, a.probe_radius, a.n_points, a.num_threads, a.chains) == ("relative_sasa", "csv", 0, 1.4, 100, 1, "")
    a = ap.parse_args(["relative-sasa", "-i", "x.pdb", "-o", "o", "-f", "z", "-t", "JSON", "-m", "2", "-r", "1.0", "-n", "50", "-j", "0", "-c", "H,L"])
    assert (a.filename, a.output_format, a.model_num, a.probe_radius, a.n_points, a.num_threads, a.chains) == ("z", "json", 2, 1.0, 50, 0, "H,L")


def test_cli_radii_flag_parses():
    ap = build_parser()
    assert ap.parse_args(["sasa", "-i", "x.pdb", "-o", "o"]).radii is None
    assert ap.parse_args(["sasa", "-i", "x.pdb", "-o", "o", "-l", "residue", "--radii", "PROTOR"]).radii == "protor"
    assert ap.parse_args(["dsasa", "-i", "x.pdb", "-g", "A/B", "--radii", "vdw"]).radii == "vdw"
    assert ap.parse_args(["dsasa", "-i", "x.pdb", "-g", "A/B"]).radii is None
    a = ap.parse_args(["sasa-ensemble", "-i", "x.pdb", "-o", "o", "-l", "residue", "--radii", "protor"])
    assert (a.level, a.radii) == ("residue", "protor")
    with pytest.raises(SystemExit):
        ap.parse_args(["sasa", "-i", "x.pdb", "-o", "o", "--radii", "chothia"])


# ---- 6. the older entry points without a table name ------------------------------------------------------------------------------------------
def test_levels_without_a_table_name_are_still_refused(tmp_path, ubq_path):
    for level in ("residue", "chain"):
        with pytest.raises(NotImplementedError):
            aa.sasa(ubq_path, level=level)
        with pytest.raises(NotImplementedError):
            aa.sasa_ensemble(ubq_path, level=level)
        assert main(["sasa", "-i", ubq_path, "-o", str(tmp_path), "-l", level]) == 2
        assert main(["sasa-ensemble", "-i", ubq_path, "-o", str(tmp_path), "-l", level]) == 2
    with pytest.raises(ValueError):
        aa.sasa(ubq_path, level="residue", radii="chothia")
    with pytest.raises(ValueError):
        aa.sasa(ubq_path, level="molecule", radii="protor")
    assert not list(tmp_path.iterdir())
