"""SASA / SAP statistics across frames (arp_sasa_ensemble): everything that is decided before the device is touched -- the CLI, the knob, the
input checks through a NULL context, the selection -- and the host-side finishing of the aggregates against its restatement."""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import ens_sasa_common as ec
import synth
from arpeggia_amd import _lib
from arpeggia_amd.api import _sasa_ensemble


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


@pytest.fixture(scope="module")
def bft(bft_path):
    return aa.load_model(bft_path)


def frames_of(s: aa.Structure, F: int) -> np.ndarray:
    return ec.topology_xyz(s)[None].repeat(F, 0)


def check(s, frames=None, chains="", probe=1.4, n_points=100, sap_radius=None):
    """The checks alone (NULL context): the selection and the frame count, or the input's error."""
    return _sasa_ensemble(None, s, frames, chains, probe, n_points, sap_radius, False)


def refused(fn, *args, match: str | None = None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == _lib.ARP_ERR_BAD_INPUT, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)
    return str(e.value)


def test_cli_defaults_and_flags(tmp_path):
    from arpeggia_amd.__main__ import build_parser

    a = build_parser().parse_args(["sasa-ensemble", "-i", "x.pdb", "-o", str(tmp_path)])
    assert (a.filename, a.output_format, a.probe_radius, a.n_points, a.num_threads, a.level, a.chains) == ("sasa_ensemble", "csv", 1.4, 100, 1, "atom", "")
    assert not hasattr(a, "model_num")
    a = build_parser().parse_args(["sasa-ensemble", "-i", "x.pdb", "-o", "d", "-f", "f", "-t", "PARQUET", "-r", "1.2", "-n", "64", "-j", "4", "-c", "A,B"])
    assert (a.filename, a.output_format, a.probe_radius, a.n_points, a.num_threads, a.chains) == ("f", "parquet", 1.2, 64, 4, "A,B")
    a = build_parser().parse_args(["sap-ensemble", "-i", "x.pdb", "-o", str(tmp_path)])
    assert (a.filename, a.output_format, a.probe_radius, a.n_points, a.sap_radius, a.num_threads, a.level, a.chains) == \
        ("sap_ensemble", "csv", 1.4, 100, 5.0, 1, "residue", "")
    assert not hasattr(a, "model_num")
    a = build_parser().parse_args(["sap-ensemble", "-i", "x.pdb", "-o", "d", "-s", "7.5", "-l", "ATOM", "-c", "H", "-n", "200", "-r", "1.0"])
    assert (a.sap_radius, a.level, a.chains, a.n_points, a.probe_radius) == (7.5, "atom", "H", 200, 1.0)
    for cmd in ("sasa-ensemble", "sap-ensemble"):
        with pytest.raises(SystemExit):
            build_parser().parse_args([cmd, "-i", "x.pdb", "-o", "d", "-m", "1"])  # no --model: the models are the frames


def test_cli_missing_input_and_level(tmp_path, ubq_path):
    from arpeggia_amd.__main__ import main

    assert main(["sasa-ensemble", "-i", str(tmp_path / "none.pdb"), "-o", str(tmp_path)]) == 1
    assert main(["sap-ensemble", "-i", str(tmp_path / "none.pdb"), "-o", str(tmp_path)]) == 1
    assert main(["sasa-ensemble", "-i", ubq_path, "-o", str(tmp_path), "-l", "residue"]) == 2


def test_chunk_knob():
    aa.debug_set("ens_chunk_atoms", 1000)
    aa.debug_set("ens_chunk_atoms", 0)
    refused(aa.debug_set, "ens_chunk_atoms", -1, match="ens_chunk_atoms")
    msg = refused(aa.debug_set, "no_such_key", 1, match="unknown key")
    assert "ens_chunk_atoms" in msg and "freq_chunk_atoms" in msg


def test_exported_names_and_columns():
    assert {"arp_sasa_ensemble", "arp_sasa_ensemble_stats"} <= set(_lib.EXPORTS)
    assert aa.ENSEMBLE_SASA_COLUMNS[:7] == ["chain", "resn", "resi", "insertion", "altloc", "atomn", "atomi"]
    assert aa.ENSEMBLE_SASA_COLUMNS[7:] == ["n_frames", "mean_sasa", "std_sasa", "min_sasa", "max_sasa"]
    assert aa.ENSEMBLE_SAP_COLUMNS == aa.ENSEMBLE_SASA_COLUMNS + ["mean_sap", "std_sap", "min_sap", "max_sap"]
    assert aa.RESIDUE_ENSEMBLE_SAP_COLUMNS == aa.api.RESIDUE_SAP_COLUMNS + ["n_frames"]
    for name in ("get_sasa_ensemble", "get_sap_ensemble", "get_residue_sap_ensemble", "sasa_ensemble", "sap_ensemble"):
        assert callable(getattr(aa, name))
    assert callable(aa.Context.sasa_ensemble)


def test_zero_frames(ubq):
    refused(check, ubq, frames_of(ubq, 0), match="at least one frame")
    refused(aa.get_sasa_ensemble, ubq, frames_of(ubq, 0), match="at least one frame")  # also ahead of a missing device


@pytest.mark.parametrize("shape", [(2, 5, 3), (2, 660, 2), (660, 3), (1, 2, 660, 3)])
def test_wrong_shape(ubq, shape):
    refused(check, ubq, np.zeros(shape), match="shape")
    refused(aa.get_sap_ensemble, ubq, np.zeros(shape), match="shape")


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinate_of_a_selected_atom(ubq, value):
    f = frames_of(ubq, 3)
    sel = aa.sasa_select(ubq)
    assert 17 in sel
    f[2, 17, 1] = value
    refused(check, ubq, f, match="frame 2, atom 17")
    refused(aa.get_sasa_ensemble, ubq, f, match="frame 2, atom 17")


def test_non_finite_coordinate_of_an_unselected_atom_is_not_an_error(ubq):
    f = frames_of(ubq, 2)
    water = int(np.flatnonzero(ubq.strings("resn") == b"HOH")[0])
    f[1, water, 0] = np.nan
    assert len(check(ubq, f)["atoms"]) == 602
    f2 = frames_of(ubq, 2)
    f2[1, int(np.flatnonzero(ubq.strings("chain") == b"A")[0]), 0] = np.nan
    assert len(check(ubq, f2, chains="Z")["atoms"]) == 0  # nothing selected: nothing to check


@pytest.mark.parametrize("n_points", [0, -5, 4097])
def test_bad_n_points(ubq, n_points):
    refused(check, ubq, frames_of(ubq, 1), n_points=n_points, match="n_points must be 1..4096")


@pytest.mark.parametrize("probe", [-0.1, np.nan, np.inf])
def test_bad_probe(ubq, probe):
    refused(check, ubq, frames_of(ubq, 1), probe=probe, match="probe radius")


@pytest.mark.parametrize("radius", [-1.0, np.nan])
def test_bad_sap_radius(ubq, radius):
    refused(check, ubq, frames_of(ubq, 1), sap_radius=radius, match="sap_radius")
    assert check(ubq, frames_of(ubq, 1), sap_radius=0.0)["n_frames"] == 1


def _models(rec: dict, F: int) -> dict:
    parts = []
    for m in range(F):
        r = {k: v.copy() for k, v in rec.items()}
        r["model_serial"][:] = m + 1
        parts.append(r)
    return {k: np.concatenate([p[k] for p in parts]) for k in rec}


def test_models_are_the_frames_and_must_agree(tmp_path, ubq_path):
    rec = synth.read_pdb_records(ubq_path)
    multi = _models(rec, 3)
    good = tmp_path / "good.pdb"
    synth.write_pdb(multi, good)
    s = aa.load_model(str(good))
    r = check(s)
    assert r["n_frames"] == 3 and len(r["atoms"]) == 602 and r["atoms"].max() < 660  # model 0's atoms only, MODEL serials 1..3 notwithstanding
    n = len(rec["x"])
    multi["name"][2 * n + 5] = b"CX"  # model 2 (MODEL 3), atom 5
    bad = tmp_path / "differ.pdb"
    synth.write_pdb(multi, bad)
    sb = aa.load_model(str(bad))
    msg = refused(check, sb, match="model 2 (MODEL 3)")
    assert "atom 5" in msg and "atom name" in msg
    try:
        aa.api._freq_table(None, sb, None, "/", 0.1, 6.5)
        raise AssertionError("the frequency path accepted the file")
    except aa.ArpeggiaError as e:
        assert str(e) == msg  # the same check, the same text
    refused(aa.sasa_ensemble, str(bad), match="model 2 (MODEL 3)")
    refused(aa.sap_ensemble, str(bad), match="model 2 (MODEL 3)")
    # with coordinates given, the structure's further models are not looked at
    assert check(sb, np.zeros((2, n, 3)))["n_frames"] == 2


@pytest.mark.parametrize("which,chains", [("ubq", ""), ("ubq", "A"), ("ubq", "Q"), ("bft", ""), ("bft", "H,L"), ("bft", " A , ")])
def test_selection_is_steps_1_to_3(request, which, chains):
    s = request.getfixturevalue(which)
    r = check(s, frames_of(s, 2), chains=chains)
    want = aa.sasa_select(s, chains, 0)  # (single-model files with MODEL serial 0: steps 4 and 5 drop nothing)
    assert np.array_equal(r["atoms"], want) and r["atoms"].dtype == np.uint32
    assert r["n_frames"] == 2
    assert not (s.strings("element")[r["atoms"]] == b"H").any() and not (s.strings("resn")[r["atoms"]] == b"HOH").any()


def test_selection_drops_hydrogens_of_a_stress_topology():
    s = aa.Structure.from_records(synth.gen_stress(n_res=40, seed=5, hydrogens=True, altlocs=True))
    r = check(s, frames_of(s, 1))
    elem = s.strings("element")
    assert (elem == b"H").any()
    assert np.array_equal(r["atoms"], np.flatnonzero((elem != b"H") & (s.strings("resn") != b"HOH")).astype(np.uint32))


def test_level_is_checked():
    with pytest.raises(ValueError):
        aa.sap_ensemble("x.pdb", level="chain")


# ---- the aggregates' finishing (arp_sasa_ensemble_stats) against the restatement with Python integers --------------------------------------
def _accumulators(counts):
    c = counts.astype(np.int64)
    return (c.sum(0).astype(np.uint64), (c * c).sum(0).astype(np.uint64), counts.min(0).astype(np.int32), counts.max(0).astype(np.int32))


@pytest.mark.parametrize("F,m,n_points,seed", [(1, 40, 100, 0), (2, 64, 1, 1), (7, 300, 65, 2), (64, 200, 100, 3), (1000, 50, 960, 4), (3, 30, 4096, 5)])
def test_sasa_aggregates_match_the_restatement(F, m, n_points, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, n_points + 1, size=(F, m)).astype(np.int32)
    counts[:, 0] = 0                      # buried in every frame
    counts[:, 1] = n_points               # fully exposed in every frame
    counts[:, 2] = counts[0, 2]           # constant
    R = (rng.choice(np.array([1.5, 1.66, 1.77, 1.89], np.float32), size=m) + np.float32(1.4)).astype(np.float32)
    got = aa.sasa_ensemble_stats(F, R, n_points, *_accumulators(counts))
    want = ec.sasa_stats(F, R, n_points, counts)
    for k in want:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k]), k
    assert (got["std_sasa"][:3] == 0).all() and got["mean_sasa"][0] == 0 and got["min_sasa"][1] == got["max_sasa"][1] == got["mean_sasa"][1]
    # min / max are the per-frame values of those counts: f32(((4 pi R) R count) / n) as the SASA kernel forms it
    b = (ec.FOUR_PI * R.astype(np.float64)) * R.astype(np.float64)
    assert np.array_equal(got["min_sasa"], (b * counts.min(0) / float(n_points)).astype(np.float32))
    assert (got["min_sasa"] <= got["mean_sasa"]).all() and (got["mean_sasa"] <= got["max_sasa"]).all()


def test_sasa_aggregates_with_accumulators_beyond_53_bits():
    """S1^2 and F S2 near 2^96: the difference is formed in 128-bit integers, not in f64."""
    F, c = 1 << 36, 4096
    s1 = np.array([F * c - 1, F * c], np.uint64)                # one frame of the first atom has count 4095
    s2 = np.array([(F - 1) * c * c + 4095 * 4095, F * c * c], np.uint64)
    R = np.array([3.17, 3.17], np.float32)
    got = aa.sasa_ensemble_stats(F, R, 4096, s1, s2, np.array([4095, 4096], np.int32), np.array([4096, 4096], np.int32))
    d = F * int(s2[0]) - int(s1[0]) ** 2
    assert d == F - 1
    import math

    r = float(R[0])
    assert got["std_sasa"][0] == np.float32((ec.FOUR_PI * r) * r * math.sqrt(float(d)) / 4096.0 / float(F)) and got["std_sasa"][0] > 0
    assert got["std_sasa"][1] == 0


@pytest.mark.parametrize("F,m,seed", [(1, 20, 0), (5, 100, 1), (257, 40, 2)])
def test_sap_aggregates_match_the_restatement(F, m, seed):
    rng = np.random.default_rng(seed)
    sap = rng.normal(scale=3.0, size=(F, m)).astype(np.float32)
    sap[:, 0] = 0.0
    sap[:, 1] = np.float32(-2.71828)
    w = ec.sap_stats(sap)
    R = np.full(m, 3.17, np.float32)
    z = np.zeros(m, np.uint64)
    got = aa.sasa_ensemble_stats(F, R, 100, z, z, np.zeros(m, np.int32), np.zeros(m, np.int32), w["t1"], w["t2"])
    assert np.array_equal(got["mean_sap"], w["mean_sap"]) and np.array_equal(got["std_sap"], w["std_sap"])
    assert got["mean_sap"][0] == 0 and got["std_sap"][0] == 0 and got["mean_sap"][1] == np.float32(-2.71828)
    assert np.allclose(got["std_sap"][2:], sap[:, 2:].astype(np.float64).std(0), rtol=1e-4, atol=1e-6)


def test_stats_reject_bad_arguments():
    z = np.zeros(2, np.uint64)
    i = np.zeros(2, np.int32)
    R = np.ones(2, np.float32)
    refused(aa.sasa_ensemble_stats, 0, R, 100, z, z, i, i, match="positive")
    refused(aa.sasa_ensemble_stats, 3, R, 0, z, z, i, i, match="positive")
