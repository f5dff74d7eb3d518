"""Secondary structure (arp_dssp) on the device.

k_dssp_pack / k_dssp_sweep / k_dssp_assign against the host twin arp_dssp_host on every case of tests/dssp_cases.py (each keeps 10^-6 from every threshold of
the definition, so the two must agree exactly): the two files, jittered frames, the built helices, R = 1 .. 5 and R around the sweep's tile; identical bytes
from call to call and from pass size to pass size; rigid motion; the identities between the outputs; the models of a structure as frames; errors; the command
line.  Expected values never come from the call under test, except where bit-equality between two calls is the property.

Inputs ON the thresholds (one ulp either side of E = -0.5, |CA - CA| = 9, |C - N| = 2.5, a distance of 0.5, kappa = 70 degrees) and features placed on the sweep's
tiles of 64 and the assignment's stride of 256 are in tests/test_dssp_edge_gpu.py (cases: tests/dssp_edge_cases.py).
"""
from __future__ import annotations

import csv
from functools import lru_cache

import numpy as np
import pytest

import arpeggia_amd as aa
import dssp_cases as dc

pytestmark = pytest.mark.gpu

KNOBS = ("rmsd_chunk_atoms",)
OUTPUTS = ("codes", "counts", "frame_counts", "hb_acceptor", "hb_energy", "fraction")
CASES = sorted(dc.device_cases())


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


@lru_cache(maxsize=None)
def host(name: str) -> dict:
    """The host twin on a case, computed once."""
    case = dc.device_cases()[name]
    return aa.secondary_structure_host(case["xyz"], case["flags"])


def device(ctx, case: dict, **kw) -> dict:
    s = aa.Structure.from_records(dc.records(case))
    sel = aa.backbone_select(s)
    R = len(case["res"])
    assert np.array_equal(sel["bb"], np.arange(4 * R).reshape(R, 4)) and np.array_equal(sel["flags"], case["flags"])
    kw.setdefault("hbonds", True)
    return ctx.secondary_structure(s, dc.frames_of(case), **kw)


def assert_equal(got: dict, want: dict, what):
    for key in ("codes", "counts", "frame_counts", "hb_acceptor"):
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5].tolist())
    g, w = got["hb_energy"], want["hb_energy"]
    ulp = np.spacing(np.maximum(np.abs(g), np.abs(w)).astype(np.float32))
    assert (np.abs(g.astype(np.float64) - w) <= 4.0 * ulp).all(), (what, "hb_energy", float(np.abs(g.astype(np.float64) - w).max()))


def same_bytes(a: dict, b: dict, what):
    for key in OUTPUTS:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


@pytest.mark.parametrize("name", CASES)
def test_device_equals_host(ctx, name):
    case = dc.device_cases()[name]
    got = device(ctx, case)
    assert_equal(got, host(name), name)
    F, R = case["xyz"].shape[:2]
    assert got["codes"].shape == (F, R) and got["hb_acceptor"].shape == (F, R, 2)


def test_pinned_results_on_the_device(ctx):
    assert aa.ss_string(device(ctx, dc.device_cases()["1ubq"])["codes"][0]) == dc.UBQ_STRING
    assert device(ctx, dc.device_cases()["6bft"])["frame_counts"][0].tolist() == dc.BFT_COUNTS
    for kind, code in (("alpha", "H"), ("310", "G"), ("pi", "I")):
        assert aa.ss_string(device(ctx, dc.device_cases()[f"helix_{kind}"])["codes"][0]) == "-" + code * 10 + "-"


def test_pass_size_and_repeat_give_the_same_bytes(ctx):
    """1ubq x 33 frames (304 backbone atoms each) in 1, 2 and 33 upload passes, and twice in a row: every output byte for byte."""
    case = dc.device_cases()["1ubq_jitter33"]
    N = 4 * len(case["res"])
    first = device(ctx, case)
    same_bytes(device(ctx, case), first, "repeat")
    for per, passes in ((17, 2), (1, 33)):
        assert -(-33 // per) == passes
        aa.debug_set("rmsd_chunk_atoms", per * N)
        same_bytes(device(ctx, case), first, passes)
    assert_equal(first, host("1ubq_jitter33"), "33 frames")
    assert len({row.tobytes() for row in first["codes"]}) > 1    # the frames do differ


def test_rigid_motion_keeps_the_codes(ctx):
    ubq = dc.device_cases()["1ubq"]
    for moved in (dc.tumbled(ubq, 5), dc.translated(ubq, 1.0e4)):
        got = device(ctx, moved)
        assert [aa.ss_string(row) for row in got["codes"]] == [dc.UBQ_STRING] * len(got["codes"])
        assert (got["hb_acceptor"] == got["hb_acceptor"][:1]).all()


def test_identities_between_the_outputs(ctx):
    case = dc.device_cases()["1ubq_jitter33"]
    F, R = case["xyz"].shape[:2]
    full = device(ctx, case)
    bare = device(ctx, case, codes=False, hbonds=False)
    assert "codes" not in bare and "hb_acceptor" not in bare and "hb_energy" not in bare
    assert np.array_equal(bare["counts"], full["counts"]) and np.array_equal(bare["frame_counts"], full["frame_counts"])
    assert (full["counts"].sum(1) == F).all() and (full["frame_counts"].sum(1) == R).all()
    hist = np.stack([(full["codes"] == k).sum(0) for k in range(8)], 1)
    assert np.array_equal(full["counts"], hist)
    assert np.array_equal(full["frame_counts"], np.stack([(full["codes"] == k).sum(1) for k in range(8)], 1))
    assert full["fraction"].dtype == np.float32 and np.abs(full["fraction"].astype(np.float64).sum(1) - 1.0).max() <= 8 * 2.0 ** -24
    assert np.array_equal(full["fraction"], (full["counts"] / F).astype("<f4"))
    assert np.array_equal(full["residue"], np.arange(R) * 4)


def test_models_are_the_frames(ctx):
    case = dc.jittered(dc.device_cases()["helix_alpha"], 5, 3)
    models = aa.Structure.from_records(dc.model_records(case))
    got = ctx.secondary_structure(models, None, hbonds=True)
    same_bytes(got, device(ctx, case), "models")
    assert got["codes"].shape == (5, dc.HELIX_RESIDUES)


def test_files_end_to_end_and_the_command_line(ctx, tmp_path):
    from arpeggia_amd.__main__ import main

    res = aa.secondary_structure(str(dc.DATA / "1ubq.pdb"))
    assert aa.ss_string(res["codes"][0]) == dc.UBQ_STRING and res["counts"].sum(0).tolist() == dc.UBQ_COUNTS
    heavy = aa.get_secondary_structure(aa.Structure.load(str(dc.DATA / "6bft.pdb")), chains="H,L", codes=False)
    assert heavy["counts"].shape[1] == 8 and "codes" not in heavy
    out = tmp_path / "out"
    assert main(["secondary-structure", "-i", str(dc.DATA / "1ubq.pdb"), "-o", str(out), "--codes", str(tmp_path / "codes.npy"), "--strings", str(tmp_path / "ss.txt")]) == 0
    with open(out / "secondary_structure.csv", newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == aa.SS_COLUMNS and len(lines) == 77
    assert "".join(row[-1] for row in lines[1:]) == dc.UBQ_STRING
    assert [row[2] for row in lines[1:]] == [str(k) for k in range(1, 77)]
    assert [float(row[5]) for row in lines[1:]] == [1.0 if c == "H" else 0.0 for c in dc.UBQ_STRING]    # frac_H of the one frame
    assert (tmp_path / "ss.txt").read_text() == dc.UBQ_STRING + "\n"
    assert np.load(tmp_path / "codes.npy").tobytes() == res["codes"].tobytes()
    assert main(["secondary-structure", "-i", str(dc.DATA / "1ubq.pdb")]) == 1    # nothing to write


def test_errors_through_python(ctx):
    case = dc.device_cases()["helix_alpha"]
    s = aa.Structure.from_records(dc.records(case))
    frames = dc.frames_of(case).copy()
    with pytest.raises(aa.ArpeggiaError, match=r"dssp: frames must have shape \[F, 48, 3\]"):
        ctx.secondary_structure(s, frames[:, :40])
    frames[0, 9, 2] = np.inf
    with pytest.raises(aa.ArpeggiaError, match="non-finite coordinate in frame 0, atom 9"):
        ctx.secondary_structure(s, frames)
    with pytest.raises(aa.ArpeggiaError, match="at least one frame is needed"):
        ctx.secondary_structure(s, frames[:0])
    with pytest.raises(aa.ArpeggiaError, match=r"dssp: no residues \(n_res == 0\)"):
        ctx.secondary_structure(s, None, chains="Z")
