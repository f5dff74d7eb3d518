"""Atom SASA, SAP score and dSASA on the MI355X (include/arpeggia_amd.h "atom SASA"): exact counts against the numpy restatement of the
contract (tests/sasa_restatement.py), analytic cases, the reference's own regression facts (src/sasa.rs tests) and the SAP chain."""
import numpy as np
import pytest

import arpeggia_amd as aa
import oracle_binding as ob
import sasa_restatement as sr
import synth
from arpeggia_amd import _lib
from conftest import DATA

pytestmark = pytest.mark.gpu

UBQ, BFT, HAND7 = str(DATA / "1ubq.pdb"), str(DATA / "6bft.pdb"), str(DATA / "hand7.pdb")


@pytest.fixture(scope="module")
def ctx():
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


def _vdw(elements) -> np.ndarray:
    p = aa.default_params()
    return np.array([p.vdw_radius[_lib.lib.arp_element_class(e)] for e in elements], dtype=np.float32)


def _structure_inputs(s, sel):
    soa = s.soa()
    return soa["x"][sel], soa["y"][sel], soa["z"][sel], _vdw(s.strings("element")[sel])


def _expected(x, y, z, r, probe, n_points, homes=None):
    R = (r + np.float32(probe)).astype(np.float32)
    counts = sr.atom_counts(x, y, z, R, aa.sasa_sphere_points(n_points), homes=homes)
    return counts, sr.sasa_from_counts(R if homes is None else R[homes], counts, n_points)


def _check_structure(s, probe=1.4, n_points=100, model_num=0, chains=""):
    idx, sasa, count = aa.api.atom_sasa_rows(s, probe, n_points, model_num, True, chains)
    sel = aa.sasa_select(s, chains, model_num)
    order = np.argsort(s.ints("atomi")[sel], kind="stable")
    assert idx.tolist() == sel[order].tolist()
    x, y, z, r = _structure_inputs(s, sel)
    want_c, want_s = _expected(x, y, z, r, probe, n_points)
    assert count.tolist() == want_c[order].tolist()
    assert sasa.view(np.uint32).tolist() == want_s[order].view(np.uint32).tolist()
    return sasa


@pytest.mark.parametrize("path,model_num", [(UBQ, 0), (BFT, 0), (HAND7, 1), (HAND7, 2)])
def test_counts_bit_identical_on_files(ctx, path, model_num):
    sasa = _check_structure(aa.load_model(path), model_num=model_num)
    assert len(sasa) > 0 and (sasa > 0).any() and (sasa == 0).any()


@pytest.mark.parametrize("n_atoms", [40_000, 100_000])
def test_counts_bit_identical_on_s1_clouds(ctx, n_atoms):
    rec = synth.gen_s1(n_atoms)
    r = _vdw(rec["element"])
    sasa, count = aa.atom_sasa(ctx, rec["x"], rec["y"], rec["z"], r, probe=1.4, n_points=100)
    want_c, want_s = _expected(rec["x"], rec["y"], rec["z"], r, 1.4, 100)
    assert np.array_equal(count, want_c)
    assert np.array_equal(sasa.view(np.uint32), want_s.view(np.uint32))


@pytest.mark.parametrize("n_points", [1, 63, 64, 100, 257])
@pytest.mark.parametrize("probe", [0.0, 1.0, 1.4, 2.0])
def test_parameter_sweep_on_1ubq(ctx, n_points, probe):
    _check_structure(aa.load_model(UBQ), probe=probe, n_points=n_points)


def test_repeat_gives_the_same_bits(ctx):
    s = aa.load_model(BFT)
    a = aa.api.atom_sasa_rows(s)
    b = aa.api.atom_sasa_rows(s)
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def test_forced_y_strips_change_nothing(ctx):
    rec = synth.gen_s1(40_000)
    r = _vdw(rec["element"])
    base = aa.atom_sasa(ctx, rec["x"], rec["y"], rec["z"], r)
    aa.debug_set("strip_rows", 4)
    try:
        strips = aa.atom_sasa(ctx, rec["x"], rec["y"], rec["z"], r)
        ubq = aa.api.atom_sasa_rows(aa.load_model(UBQ))
    finally:
        aa.debug_set("strip_rows", 0)
    assert np.array_equal(base[1], strips[1]) and np.array_equal(base[0].view(np.uint32), strips[0].view(np.uint32))
    assert np.array_equal(ubq[2], aa.api.atom_sasa_rows(aa.load_model(UBQ))[2])


def test_million_atoms_against_a_seeded_sample(ctx):
    rec = synth.gen_s1(1_000_000)
    r = _vdw(rec["element"])
    sasa, count = aa.atom_sasa(ctx, rec["x"], rec["y"], rec["z"], r)
    homes = np.sort(np.random.default_rng(20261015).choice(len(r), 20_000, replace=False))
    want_c, want_s = _expected(rec["x"], rec["y"], rec["z"], r, 1.4, 100, homes=homes)
    assert np.array_equal(count[homes], want_c)
    assert np.array_equal(sasa[homes].view(np.uint32), want_s.view(np.uint32))
    assert aa.sasa_tests(ctx) > 0


def test_analytic_cases(ctx):
    one = np.array([1.7], np.float32)
    sasa, count = aa.atom_sasa(ctx, [1.0], [2.0], [3.0], one, probe=1.4, n_points=100)
    R = np.float32(np.float32(1.7) + np.float32(1.4))
    assert count.tolist() == [100] and sasa[0] == np.float32(4.0 * np.pi * float(R) * float(R))
    # two atoms exactly R_i + R_j apart along x (representable: R = 2 + 1 = 3, centres 6 apart): nothing is buried -- but not because the test is
    # strict: no golden-spiral point lies on the x axis (point 0 is the pole (0, 0, 1) for every n_points), so no point touches the other sphere
    sasa, count = aa.atom_sasa(ctx, [0.0, 6.0], [0.0, 0.0], [0.0, 0.0], np.array([2.0, 2.0], np.float32), probe=1.0, n_points=1)
    assert count.tolist() == [1, 1]
    sasa, count = aa.atom_sasa(ctx, [0.0, 6.0], [0.0, 0.0], [0.0, 0.0], np.array([2.0, 2.0], np.float32), probe=1.0, n_points=64)
    assert count.tolist() == [64, 64]
    # the strict edge: along z point 0 of the lower atom sits at d^2 == R_j^2 exactly -- open; one f32 step closer it is buried
    closer = float(np.nextafter(np.float32(6.0), np.float32(0.0)))
    for n_points, full in ((1, 1), (64, 64)):
        sasa, count = aa.atom_sasa(ctx, [0.0, 0.0], [0.0, 0.0], [0.0, 6.0], np.array([2.0, 2.0], np.float32), probe=1.0, n_points=n_points)
        assert count.tolist() == [full, full]
        sasa, count = aa.atom_sasa(ctx, [0.0, 0.0], [0.0, 0.0], [0.0, closer], np.array([2.0, 2.0], np.float32), probe=1.0, n_points=n_points)
        assert count.tolist() == [full - 1, full]
    sasa, count = aa.atom_sasa(ctx, [0.0, 0.0], [0.0, 0.0], [100.0, 110.5], np.array([0.5, 10.0], np.float32), probe=0.0, n_points=1)
    assert count.tolist() == [1, 1]
    sasa, count = aa.atom_sasa(ctx, [0.0, 0.0], [0.0, 0.0], [100.0, float(np.nextafter(np.float32(110.5), np.float32(0.0)))], np.array([0.5, 10.0], np.float32),
                               probe=0.0, n_points=1)
    assert count.tolist() == [0, 1]
    # an atom inside a much larger one
    sasa, count = aa.atom_sasa(ctx, [0.0, 0.5], [0.0, 0.0], [0.0, 0.0], np.array([10.0, 1.0], np.float32), probe=1.4, n_points=100)
    assert count[1] == 0 and sasa[1] == 0.0 and count[0] == 100
    # excluded atoms neither bury nor get a value
    sasa, count = aa.atom_sasa(ctx, [0.0, 0.5], [0.0, 0.0], [0.0, 0.0], np.array([10.0, 1.0], np.float32), include=[0, 1], n_points=100)
    assert count.tolist() == [0, 100]
    # empty input / empty selection
    sasa, count = aa.atom_sasa(ctx, [], [], [], np.zeros(0, np.float32))
    assert len(sasa) == 0
    t = aa.get_atom_sasa(aa.load_model(HAND7), model_num=0)
    assert len(t) == 0 and _cols(t) == aa.api.ATOM_SASA_COLUMNS
    for kw in (dict(n_points=0), dict(n_points=_lib.ARP_SASA_MAX_POINTS + 1), dict(probe=-0.1), dict(probe=float("nan")), dict(probe=float("inf"))):
        with pytest.raises(aa.ArpeggiaError) as e:
            aa.atom_sasa(ctx, [0.0], [0.0], [0.0], one, **kw)
        assert e.value.status == _lib.ARP_ERR_BAD_INPUT
    with pytest.raises(aa.ArpeggiaError) as e:
        aa.atom_sasa(ctx, [0.0], [0.0], [0.0], np.array([np.nan], np.float32))
    assert e.value.status == _lib.ARP_ERR_BAD_INPUT


def _cols(t):
    return list(t.columns) if hasattr(t, "columns") and not hasattr(t, "column_names") else list(t.column_names)


def _col(t, name):
    return np.asarray(t[name].to_numpy() if hasattr(t[name], "to_numpy") else t.column(name).to_numpy())


def test_reference_facts(ctx):
    t = aa.sasa(UBQ)
    assert _cols(t) == aa.api.ATOM_SASA_COLUMNS and len(t) == 602
    total = float(_col(t, "sasa").astype(np.float64).sum())
    assert abs(total - 4813.0) <= 100.0, total  # sasa.rs test_sasa_regression_ubiquitin
    assert (np.diff(_col(t, "atomi")) > 0).all()
    d = aa.dsasa(BFT, "C/H,L")
    assert abs(d - 1650.0) <= 50.0, d  # sasa.rs test_get_dsasa_interface_value
    a, b = aa.dsasa(BFT, "A,B,C/G,H,L"), aa.dsasa(BFT, "G,H,L/A,B,C")
    assert a > 0 and a == b
    t1, t2 = aa.sasa(UBQ, probe_radius=1.0), aa.sasa(UBQ, probe_radius=2.0)
    assert _col(t1, "sasa").astype(np.float64).sum() > _col(t2, "sasa").astype(np.float64).sum()  # test_sasa_probe_radius_effect
    with pytest.raises(aa.ArpeggiaError) as e:
        aa.dsasa(BFT, "A,B")
    assert e.value.status == _lib.ARP_ERR_BAD_GROUPS
    sap = aa.sap_score(UBQ, level="atom")
    assert _cols(sap) == aa.api.ATOM_SAP_COLUMNS
    v = _col(sap, "sap_score")
    assert (v > 0).any() and (v < 0).any()
    res = aa.sap_score(UBQ)
    assert _cols(res) == aa.api.RESIDUE_SAP_COLUMNS and len(res) > 0 and (_col(res, "sap_score") > 0).all()


@pytest.mark.parametrize("path,chains", [(UBQ, ""), (BFT, "H,L"), (BFT, "")])
def test_sap_matches_the_restatement(ctx, path, chains):
    s = aa.load_model(path)
    idx, sasa, sap = aa.api.atom_sap_rows(s, chains=chains)
    rows_idx, rows_sasa, _ = aa.api.atom_sasa_rows(s, chains=chains)
    # the neighbour set: chain filter, H and solvent removal, no model filter (sap.rs:182)
    nb = aa.sasa_select(s, chains, model_num=0)  # (single-model files with serial 0: steps 1-5 = steps 1-3)
    soa = s.soa()
    serial, names, resn = s.ints("atomi"), s.strings("atomn"), s.strings("resn")
    score, side = sr.per_atom_sap({"serial": serial[rows_idx], "sasa": rows_sasa, "resn": resn[rows_idx]},
                                  {"x": soa["x"][nb], "y": soa["y"][nb], "z": soa["z"][nb], "serial": serial[nb], "name": names[nb], "resn": resn[nb]},
                                  5.0, ob.sap_weight, ob.sap_neighbor_sum)
    score_of = {int(serial[nb[k]]): score[k] for k in range(len(nb)) if side[k]}
    non_bb = set(serial[~np.isin(names, sr.BACKBONE)].tolist())
    want_idx = [i for i in rows_idx if int(serial[i]) in non_bb]
    assert idx.tolist() == want_idx
    want = np.array([score_of.get(int(serial[i]), 0.0) for i in want_idx], np.float32)
    assert np.abs(sap - want).max() <= 2e-5 * max(1.0, float(np.abs(want).max()))
    # per residue: the group-by of the restated scores, row for row
    t = aa.get_per_residue_sap_score(s, chains=chains)
    dec = lambda a: [v.decode() for v in a]  # noqa: E731
    keys, sc, sp, mx, rel = sr.residue_group_by(dec(s.strings("chain")[idx]), dec(resn[idx]), s.ints("resi")[idx], dec(s.strings("insertion")[idx]),
                                                sasa, want, aa.api.SAP_MAX_SC_ASA)
    assert [(c, r, int(i), ic) for c, r, i, ic in zip(_col(t, "chain"), _col(t, "resn"), _col(t, "resi"), _col(t, "insertion"))] == keys
    assert np.array_equal(_col(t, "sc_sasa"), sc) and np.array_equal(_col(t, "max_sc_asa"), mx)
    assert np.abs(_col(t, "sap_score") - sp).max(initial=0.0) <= 2e-5 * max(1.0, float(np.abs(sp).max(initial=0.0)))


def test_sasa_between_contact_calls_keeps_the_table_right(ctx):
    s = aa.load_model(UBQ)
    assert len(ctx.get_contacts(s)["model"]) == 532
    aa.api.atom_sasa_rows(s)
    x, y, z, r = _structure_inputs(s, aa.sasa_select(s))
    aa.atom_sasa(ctx, x, y, z, r)
    assert len(ctx.get_contacts(s)["model"]) == 532
    assert len(aa.get_contacts(s)) == 532
