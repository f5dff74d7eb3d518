"""SASA / SAP statistics across frames (arp_sasa_ensemble) on the device, against a per-frame loop over the existing entry points.

Expected values come from aa.atom_sasa, aa.sap_weight and aa.sap_neighbor_sum called once per frame on the selected atoms -- the calls
tests/sasa_restatement.py and the oracle pin -- never from the new path.  SASA is integer counts: every count, aggregate and total must be
equal.  SAP is an f32 sum whose order follows the cell list, which differs between the packed call and a per-frame call: per-frame values are
held to the project's SAP tolerance (ens_sasa_common.SAP_TOL), and the SAP aggregates must then follow from the new path's own per-frame
values exactly.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import ens_sasa_common as ec
import synth
from ens_sasa_common import SAP_KEYS, SASA_KEYS, assert_sap_aggregates, assert_sap_close, assert_sasa_equal

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ctx():
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_chunk():
    yield
    aa.debug_set("ens_chunk_atoms", 0)


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


@pytest.fixture(scope="module")
def bft(bft_path):
    return aa.load_model(bft_path)


@pytest.fixture(scope="module")
def stress():
    return aa.Structure.from_records(synth.gen_stress(n_res=120, seed=11, hydrogens=True, altlocs=True))


# ---- one frame -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ubq", "bft"])
def test_single_frame(ctx, request, which):
    s = request.getfixturevalue(which)
    frames = ec.topology_xyz(s)[None]
    got = ctx.sasa_ensemble(s, frames, per_frame=True)
    sel = aa.sasa_select(s)
    assert np.array_equal(got["atoms"], sel) and got["n_frames"] == 1
    want = ec.frame_loop(ctx, s, sel, frames, 1.4, 100)
    assert_sasa_equal(got, want, want["R"], 100)
    assert (got["std_sasa"] == 0).all() and np.array_equal(got["min_sasa"], got["max_sasa"]) and np.array_equal(got["mean_sasa"], got["min_sasa"])
    # the structure-level call on the same single-model file, by atom index
    idx, sasa, count = aa.api.atom_sasa_rows(s)
    order = np.argsort(idx, kind="stable")
    assert np.array_equal(idx[order], got["atoms"])
    assert np.array_equal(count[order], got["count"][0]) and np.array_equal(sasa[order], got["mean_sasa"])
    assert got["total_sasa"][0] > 1000.0


# ---- jittered frames, forced passes, repeats -----------------------------------------------------------------------------------------------
# (structure, frames, chains, frames per pass for three passes, for four passes: both with a partial last pass)
CASES = [("ubq", 64, "", 25, 20), ("bft", 16, "", 6, 5), ("bft", 16, "H,L", 6, 5), ("stress", 32, "", 12, 10)]


@pytest.mark.parametrize("which,F,chains,per3,per4", CASES)
def test_jittered_frames_and_passes(ctx, request, which, F, chains, per3, per4):
    s = request.getfixturevalue(which)
    frames = ec.jittered(s, F, seed=F)
    got = ctx.sasa_ensemble(s, frames, chains, per_frame=True)
    sel = got["atoms"]
    m = len(sel)
    assert m > 0 and not (s.strings("element")[sel] == b"H").any()
    if chains:
        assert set(s.strings("chain")[sel].tolist()) == {c.encode() for c in chains.split(",")}
    want = ec.frame_loop(ctx, s, sel, frames, 1.4, 100)
    assert_sasa_equal(got, want, want["R"], 100)
    # the jitter moves the surface: the statistics are not trivially constant
    assert (got["std_sasa"] > 0).sum() > m / 2
    assert (got["min_sasa"] <= got["mean_sasa"]).all() and (got["mean_sasa"] <= got["max_sasa"]).all()
    again = ctx.sasa_ensemble(s, frames, chains, per_frame=True)
    assert ec.result_bytes(again) == ec.result_bytes(got)
    for per, passes in ((per3, 3), (per4, 4)):
        assert -(-F // per) == passes and F % per != 0
        aa.debug_set("ens_chunk_atoms", per * m)
        forced = ctx.sasa_ensemble(s, frames, chains, per_frame=True)
        assert ec.result_bytes(forced) == ec.result_bytes(got), passes
    aa.debug_set("ens_chunk_atoms", 0)
    five = ctx.sasa_ensemble(s, frames[:5], chains, per_frame=True)
    aa.debug_set("ens_chunk_atoms", 1)  # one frame per pass
    assert ec.result_bytes(ctx.sasa_ensemble(s, frames[:5], chains, per_frame=True)) == ec.result_bytes(five)


@pytest.mark.parametrize("n_points", [1, 64, 65, 100, 960])
@pytest.mark.parametrize("probe", [0.0, 1.4])
def test_points_and_probe(ctx, ubq, n_points, probe):
    frames = ec.jittered(ubq, 8, seed=n_points)
    got = ctx.sasa_ensemble(ubq, frames, "", probe, n_points, per_frame=True)
    want = ec.frame_loop(ctx, ubq, got["atoms"], frames, probe, n_points)
    assert_sasa_equal(got, want, want["R"], n_points)
    assert got["count"].max() <= n_points and got["count"].max() > 0


def test_two_thousand_frames(ctx, ubq):
    F = 2000
    frames = ec.jittered(ubq, F, seed=2000)
    got = ctx.sasa_ensemble(ubq, frames, per_frame=True)
    sel = got["atoms"]
    assert len(sel) * F > 1_200_000
    sample = sorted(np.random.default_rng(50).choice(F, size=50, replace=False).tolist())
    want = ec.frame_loop(ctx, ubq, sel, frames, 1.4, 100, which=sample)
    assert np.array_equal(got["count"][sample], want["count"])
    assert np.array_equal(got["total_sasa"][sample], ec.total_sasa(want["sasa"]))
    # the aggregates from integer accumulators over the call's own per-frame counts (whose sample the loop has just confirmed)
    stats = ec.sasa_stats(F, want["R"], 100, got["count"])
    for k in SASA_KEYS:
        assert np.array_equal(got[k], stats[k]), k
    assert (got["std_sasa"] > 0).sum() > len(sel) / 2


def _model_file(tmp_path, ubq_path, F=8):
    rec = synth.read_pdb_records(ubq_path)
    rng = np.random.default_rng(8)
    parts = []
    for m in range(F):
        r = {k: v.copy() for k, v in rec.items()}
        for ax in ("x", "y", "z"):
            r[ax] = np.round(r[ax] + rng.normal(scale=0.3, size=len(r[ax])), 3)
        r["model_serial"][:] = m + 1
        parts.append(r)
    path = tmp_path / "ubq_models.pdb"
    synth.write_pdb({k: np.concatenate([p[k] for p in parts]) for k in rec}, path)
    return path


def test_model_file_matches_arrays(ctx, tmp_path, ubq_path):
    F = 8
    s = aa.load_model(str(_model_file(tmp_path, ubq_path, F)))
    n = aa.api._topology_atoms(s)
    assert s.n_atoms == F * n
    soa = s.soa("/")
    frames = np.stack([soa["x"], soa["y"], soa["z"]], 1).reshape(F, n, 3)
    for sap_radius in (None, 5.0):
        from_models = ctx.sasa_ensemble(s, None, sap_radius=sap_radius, per_frame=True)
        from_arrays = ctx.sasa_ensemble(s, frames, sap_radius=sap_radius, per_frame=True)
        assert from_models["n_frames"] == F and ec.result_bytes(from_models) == ec.result_bytes(from_arrays)
    want = ec.frame_loop(ctx, s, from_models["atoms"], frames, 1.4, 100)
    assert_sasa_equal(from_models, want, want["R"], 100)
    assert len(from_models["atoms"]) == 602 and from_models["atoms"].max() < n


def test_empty_selection(ctx, ubq):
    frames = ec.jittered(ubq, 4, seed=4)
    for sap_radius in (None, 5.0):
        got = ctx.sasa_ensemble(ubq, frames, "Z", sap_radius=sap_radius, per_frame=True)
        assert got["n_frames"] == 4 and len(got["atoms"]) == 0 and got["count"].shape == (4, 0)
        assert all(len(got[k]) == 0 for k in SASA_KEYS) and np.array_equal(got["total_sasa"], np.zeros(4, np.float32))
    t = aa.get_sap_ensemble(ubq, frames, "Z")
    assert len(t) == 0


# ---- SAP -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,F,chains,per3,per4", CASES)
def test_sap_over_frames(ctx, request, which, F, chains, per3, per4):
    s = request.getfixturevalue(which)
    frames = ec.jittered(s, F, seed=100 + F)
    got = ctx.sasa_ensemble(s, frames, chains, sap_radius=5.0, per_frame=True)
    sel = got["atoms"]
    m = len(sel)
    want = ec.frame_loop(ctx, s, sel, frames, 1.4, 100, sap_radius=5.0)
    assert_sasa_equal(got, want, want["R"], 100)  # the weights' inputs are exact
    assert_sap_close(got["sap"], want["sap"], want["side"])
    assert_sap_aggregates(got)
    assert (got["std_sap"][want["side"]] > 0).any() and np.abs(got["mean_sap"]).max() > 0.1
    again = ctx.sasa_ensemble(s, frames, chains, sap_radius=5.0, per_frame=True)
    assert ec.result_bytes(again) == ec.result_bytes(got)
    for per in (per3, per4):
        aa.debug_set("ens_chunk_atoms", per * m)
        forced = ctx.sasa_ensemble(s, frames, chains, sap_radius=5.0, per_frame=True)
        for k in SASA_KEYS + ("count", "total_sasa"):
            assert np.array_equal(forced[k], got[k]), k
        # the contract lets SAP's last bits move with the pass size (the order of the f32 sum follows the packed grid and the kernel's split by
        # task count): the forced passes are held to the loop like the single pass, and their aggregates to their own per-frame values
        assert_sap_close(forced["sap"], want["sap"], want["side"])
        assert_sap_aggregates(forced)
        assert ec.result_bytes(ctx.sasa_ensemble(s, frames, chains, sap_radius=5.0, per_frame=True)) == ec.result_bytes(forced)


@pytest.mark.parametrize("sap_radius", [0.0, 3.0, 10.0])
def test_sap_radii(ctx, ubq, sap_radius):
    frames = ec.jittered(ubq, 6, seed=6)
    got = ctx.sasa_ensemble(ubq, frames, sap_radius=sap_radius, per_frame=True)
    want = ec.frame_loop(ctx, ubq, got["atoms"], frames, 1.4, 100, sap_radius=sap_radius)
    assert_sap_close(got["sap"], want["sap"], want["side"])
    assert_sap_aggregates(got)


def test_sap_single_frame_against_the_structure_call(ctx, ubq):
    frames = ec.topology_xyz(ubq)[None]
    got = ctx.sasa_ensemble(ubq, frames, sap_radius=5.0, per_frame=True)
    idx, sasa, sap = aa.api.atom_sap_rows(ubq)  # (serials are unique on 1ubq: the reference's by-serial maps change nothing)
    pos = {int(a): k for k, a in enumerate(got["atoms"])}
    rows = np.array([pos[int(a)] for a in idx])
    assert np.array_equal(got["mean_sasa"][rows], sasa)
    assert float(np.abs(got["mean_sap"][rows] - sap).max()) <= ec.SAP_TOL * max(1.0, float(np.abs(sap).max()))
    assert np.array_equal(got["mean_sap"], got["sap"][0]) and (got["std_sap"] == 0).all()
    assert np.array_equal(got["min_sap"], got["sap"][0]) and np.array_equal(got["max_sap"], got["sap"][0])


def _col(t, name):
    return np.asarray(t[name].to_numpy() if hasattr(t[name], "to_numpy") else t[name])


def _names(t):
    return t.column_names if hasattr(t, "column_names") else list(t.columns)  # pyarrow.Table / polars.DataFrame


def test_tables_and_residue_level(ctx, ubq):
    frames = ec.jittered(ubq, 8, seed=88)
    r = ctx.sasa_ensemble(ubq, frames, sap_radius=5.0)
    t = aa.get_sap_ensemble(ubq, frames)
    assert _names(t) == aa.ENSEMBLE_SAP_COLUMNS and len(t) == 602
    for k in SASA_KEYS + SAP_KEYS:
        assert np.array_equal(_col(t, k), r[k]), k
    assert (_col(t, "n_frames") == 8).all() and np.array_equal(_col(t, "atomi"), ubq.ints("atomi")[r["atoms"]])
    t2, extra = aa.get_sasa_ensemble(ubq, frames, per_frame=True)
    assert _names(t2) == aa.ENSEMBLE_SASA_COLUMNS
    assert np.array_equal(_col(t2, "mean_sasa"), r["mean_sasa"]) and extra["count"].shape == (8, 602) and extra["total_sasa"].shape == (8,)
    res = aa.get_residue_sap_ensemble(ubq, frames)
    idx = r["atoms"]
    dec = lambda a: [v.decode() for v in a]  # noqa: E731
    want = aa.api.residue_sap_from_atoms(dec(ubq.strings("chain")[idx]), dec(ubq.strings("resn")[idx]), ubq.ints("resi")[idx],
                                         dec(ubq.strings("insertion")[idx]), r["mean_sasa"], r["mean_sap"])
    assert _names(res) == aa.RESIDUE_ENSEMBLE_SAP_COLUMNS and len(res) == len(want["resi"]) > 0
    for k in ("sc_sasa", "sap_score", "max_sc_asa", "relative_sc_sasa", "resi"):
        assert np.array_equal(_col(res, k), want[k]), k
    assert list(_col(res, "resn")) == want["resn"]


def test_contact_calls_around_an_ensemble_call_keep_the_table_right(ctx, ubq):
    assert len(ctx.get_contacts(ubq)["model"]) == 532
    ctx.sasa_ensemble(ubq, ec.jittered(ubq, 12, seed=12), sap_radius=5.0)
    assert len(ctx.get_contacts(ubq)["model"]) == 532
    ctx.sasa_ensemble(ubq, ec.jittered(ubq, 3, seed=3))
    assert len(ctx.get_contacts(ubq)["model"]) == 532
    assert len(aa.get_contacts(ubq)) == 532


def test_cli_end_to_end(ctx, tmp_path, ubq_path):
    import csv

    from arpeggia_amd.__main__ import main

    path = _model_file(tmp_path, ubq_path, 8)
    s = aa.load_model(str(path))
    r = ctx.sasa_ensemble(s, None, sap_radius=5.0)
    out = tmp_path / "out"
    assert main(["sasa-ensemble", "-i", str(path), "-o", str(out)]) == 0
    rows = list(csv.DictReader(open(out / "sasa_ensemble.csv")))
    assert list(rows[0].keys()) == aa.ENSEMBLE_SASA_COLUMNS and len(rows) == 602
    assert np.allclose(np.array([float(x["mean_sasa"]) for x in rows]), r["mean_sasa"], rtol=1e-6, atol=0)  # (text)
    assert {x["n_frames"] for x in rows} == {"8"}
    assert main(["sap-ensemble", "-i", str(path), "-o", str(out), "-l", "atom"]) == 0
    rows = list(csv.DictReader(open(out / "sap_ensemble.csv")))
    assert list(rows[0].keys()) == aa.ENSEMBLE_SAP_COLUMNS and len(rows) == 602
    assert np.allclose(np.array([float(x["mean_sap"]) for x in rows]), r["mean_sap"], rtol=1e-6, atol=0)
    assert main(["sap-ensemble", "-i", str(path), "-o", str(out), "-f", "res"]) == 0
    rows = list(csv.DictReader(open(out / "res.csv")))
    assert list(rows[0].keys()) == aa.RESIDUE_ENSEMBLE_SAP_COLUMNS and len(rows) == len(aa.get_residue_sap_ensemble(s))
