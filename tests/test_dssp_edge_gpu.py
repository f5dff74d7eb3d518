"""Secondary structure (arp_dssp) on the device, ON its decision thresholds and launch boundaries.

Every case of tests/dssp_edge_cases.py through Context.secondary_structure: k_dssp_pack / k_dssp_sweep / k_dssp_assign must agree with the Python-float
restatement of the definition (which tests/test_dssp_edge_host.py shows to equal the host twin, and to reach every edge) where an input lies exactly on
E = -0.5, |CA - CA| = 9, |C - N| = 2.5, a distance of 0.5 or kappa = 70 degrees, or one ulp to either side; with the probes placed on either side of the sweep's
tiles of 64 and the assignment's stride of 256; with the two best acceptors arriving from different tiles in every order, tied, and clamped; with every mask
full; and with real helices, hairpins, chain starts and a proline on those boundaries.  codes, counts, frame_counts and hb_acceptor are exact, hb_energy is
within the bound of tests/test_dssp_gpu.py.  Expected values never come from the call under test, except where bit-equality between two calls is the property.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import dssp_cases as dc
import dssp_edge_cases as ec

pytestmark = pytest.mark.gpu

OUTPUTS = ("codes", "counts", "frame_counts", "hb_acceptor", "hb_energy", "fraction")


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    aa.debug_set("rmsd_chunk_atoms", 0)


def device(ctx, case: dict) -> dict:
    s = aa.Structure.from_records(dc.records(case))
    sel = aa.backbone_select(s)
    R = len(case["res"])
    assert np.array_equal(sel["bb"], np.arange(4 * R).reshape(R, 4)) and np.array_equal(sel["flags"], case["flags"])
    return ctx.secondary_structure(s, dc.frames_of(case), hbonds=True)


def assert_expected(got: dict, want: dict, what):
    for key in ("codes", "counts", "frame_counts", "hb_acceptor"):
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5].tolist())
    g, w = got["hb_energy"], want["hb_energy"]
    ulp = np.spacing(np.maximum(np.abs(g), np.abs(w)).astype(np.float32))
    assert (np.abs(g.astype(np.float64) - w) <= 4.0 * ulp).all(), (what, "hb_energy", float(np.abs(g.astype(np.float64) - w).max()))


@pytest.mark.parametrize("name", ec.NAMES)
def test_device_equals_the_restatement(ctx, name):
    case = ec.case(name)
    got = device(ctx, case)
    assert_expected(got, ec.want(name), name)
    if "string" in case:
        assert ec.strings(got["codes"]) == [case["string"]] * len(got["codes"])
    if name in ec.SWEEPS:      # every frame a pass of its own: the same bytes
        aa.debug_set("rmsd_chunk_atoms", 4 * len(case["res"]))
        alone = device(ctx, case)
        for key in OUTPUTS:
            assert alone[key].tobytes() == got[key].tobytes(), (name, key)
