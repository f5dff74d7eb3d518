"""CPU checks of the atom-SASA surface (include/arpeggia_amd.h "atom SASA"): the sphere-point table, the atom selection of
prepare_pdb_for_sasa + filter_pdb_by_model (reference src/sasa.rs:27-135,183-195) with its model quirk, the SAP tables and the CLI flags
(src/cli/{sasa,sap,dsasa}.rs).  No compute call is made."""
import numpy as np
import pytest

import arpeggia_amd as aa
import sasa_restatement as sr
from arpeggia_amd import _lib
from arpeggia_amd.__main__ import build_parser
from conftest import DATA


@pytest.mark.parametrize("n", [1, 2, 63, 64, 100, 257, 4096])
def test_sphere_points_are_the_golden_spiral(n):
    got = aa.sasa_sphere_points(n)
    assert got.dtype == np.float32 and got.shape == (n, 3)
    assert np.abs(got.astype(np.float64) - sr.sphere_points(n).astype(np.float64)).max() <= 1e-6
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert got[0].tolist() == [0.0, 0.0, 1.0]  # t = 0: the pole


def test_sphere_points_reject_bad_sizes():
    for n in (0, _lib.ARP_SASA_MAX_POINTS + 1):
        with pytest.raises(aa.ArpeggiaError) as e:
            aa.sasa_sphere_points(n)
        assert e.value.status == _lib.ARP_ERR_BAD_INPUT


def test_selection_drops_water_of_1ubq():
    s = aa.load_model(str(DATA / "1ubq.pdb"))
    sel = aa.sasa_select(s)
    assert len(sel) == 602 and s.n_atoms == 660
    assert not (s.strings("resn")[sel] == b"HOH").any()
    assert (np.diff(sel.astype(np.int64)) > 0).all()


def test_selection_chain_filter_on_6bft():
    s = aa.load_model(str(DATA / "6bft.pdb"))
    chain = s.strings("chain")
    def chains(spec):
        return sorted({c.decode() for c in chain[aa.sasa_select(s, spec)]})
    everything = sorted({c.decode() for c in chain[s.strings("resn") != b"HOH"]})
    assert chains("A") == ["A"]
    assert chains("A,B") == ["A", "B"]
    assert chains(" A , ") == ["A"]  # entries trimmed, empty entries dropped (parse_chain_string)
    assert chains("") == everything and chains(",") == everything
    assert len(aa.sasa_select(s, "A")) == int(((chain == b"A") & (s.strings("resn") != b"HOH")).sum())
    assert len(aa.sasa_select(s, "Q")) == 0


def _synthetic():
    # residue 1 ALA (with H), 2 ACE, 3 NH2, 4 NA, 5 HOH, 6 GLY: only ALA and GLY heavy atoms survive
    rows = [("ALA", "N", "N"), ("ALA", "CA", "C"), ("ALA", "H", "H"), ("ACE", "C", "C"), ("NH2", "N", "N"), ("NA", "NA", "NA"),
            ("HOH", "O", "O"), ("GLY", "CA", "C"), ("GLY", "HA2", "H")]
    res = [1, 1, 1, 2, 3, 4, 5, 6, 6]
    n = len(rows)
    rec = {"x": np.arange(n) * 4.0, "y": np.zeros(n), "z": np.zeros(n), "serial": np.arange(1, n + 1, dtype=np.int32),
           "resi": np.array(res, np.int32), "name": [r[1].encode() for r in rows], "resn": [r[0].encode() for r in rows],
           "chain": [b"A"] * n, "element": [r[2].encode() for r in rows], "res_ord": np.array(res, np.uint32) - 1,
           "res_id": np.array(res, np.uint32) - 1}
    return aa.Structure.from_records(rec, hierarchy=True)


def test_selection_drops_hydrogens_solvent_ions_and_caps():
    s = _synthetic()
    sel = aa.sasa_select(s)
    assert [(r.decode(), a.decode()) for r, a in zip(s.strings("resn")[sel], s.strings("atomn")[sel])] == [("ALA", "N"), ("ALA", "CA"), ("GLY", "CA")]
    keep_h = aa.sasa_select(s, remove_hydrogens=False)
    assert sorted(s.strings("atomn")[keep_h].tolist()) == sorted([b"N", b"CA", b"H", b"CA", b"HA2"])


def test_selection_model_quirk_on_hand7():
    """filter by MODEL serial == model_num (sasa.rs:193): the default 0 selects nothing on a file with MODEL 1..N records."""
    s = aa.load_model(str(DATA / "hand7.pdb"))
    models = s.ints("model")
    assert sorted(set(models.tolist())) == [1, 2]
    assert len(aa.sasa_select(s, model_num=0)) == 0
    for m in (1, 2):
        sel = aa.sasa_select(s, model_num=m)
        assert len(sel) > 0 and set(models[sel].tolist()) == {m}
        want = (models == m) & (s.strings("resn") != b"HOH") & (s.strings("element") != b"H")
        assert sorted(sel.tolist()) == np.flatnonzero(want).tolist()
    assert len(aa.sasa_select(s, model_num=3)) == 0  # no such model: the first is kept, then nothing matches serial 3
    # and the other half of the quirk: model_num 1 on a file without MODEL records
    u = aa.load_model(str(DATA / "1ubq.pdb"))
    assert len(aa.sasa_select(u, model_num=1)) == 0


def test_sap_tables_agree_with_the_weight_function():
    for resn, mx in aa.api.SAP_MAX_SC_ASA.items():
        h = aa.sap_weight(resn, mx * 4)  # clamped to 1
        assert aa.sap_weight(resn, np.float32(mx)) == h
        assert aa.sap_weight(resn, 0.0) == 0.0
    assert aa.sap_weight("HOH", 50.0) == 0.0


def test_cli_carries_the_reference_flags():
    ap = build_parser()
    a = ap.parse_args(["sasa", "-i", "x.pdb", "-o", "out"])
    assert (a.filename, a.output_format, a.model_num, a.probe_radius, a.n_points, a.num_threads, a.level, a.chains) == ("sasa", "csv", 0, 1.4, 100, 1, "atom", "")
    a = ap.parse_args(["sap", "-i", "x.pdb", "-o", "out"])
    assert (a.filename, a.output_format, a.model_num, a.probe_radius, a.n_points, a.sap_radius, a.num_threads, a.level, a.chains) == \
        ("sap", "csv", 0, 1.4, 100, 5.0, 1, "residue", "")
    a = ap.parse_args(["dsasa", "-i", "x.pdb", "-g", "A/B"])
    assert (a.groups, a.model_num, a.probe_radius, a.n_points, a.num_threads) == ("A/B", 0, 1.4, 100, 1)
    a = ap.parse_args(["sap", "-i", "x.pdb", "-o", "o", "-m", "2", "-r", "1.0", "-n", "50", "-s", "7.5", "-j", "0", "-l", "atom", "-c", "H,L", "-t", "json", "-f", "z"])
    assert (a.model_num, a.probe_radius, a.n_points, a.sap_radius, a.num_threads, a.level, a.chains, a.output_format, a.filename) == \
        (2, 1.0, 50, 7.5, 0, "atom", "H,L", "json", "z")


def test_python_levels_outside_the_atom_level_are_refused():
    with pytest.raises(NotImplementedError):
        aa.sasa(str(DATA / "1ubq.pdb"), level="residue")
    with pytest.raises(ValueError):
        aa.sasa(str(DATA / "1ubq.pdb"), level="molecule")
    with pytest.raises(ValueError):
        aa.sap_score(str(DATA / "1ubq.pdb"), level="chain")
