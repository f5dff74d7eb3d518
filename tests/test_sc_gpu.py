"""Shape complementarity on the device against the sequential C restatement (tests/sc_restatement.c), dot for dot.

Counts, kinds and the buried / trimmed flags must be EQUAL and in the same order; positions, normals, areas, nn_dist and scores agree
within 1e-9 relative; sc, distance and area within 1e-12.  The only expected difference is the device library's sin / cos / atan2 / acos
/ exp against glibc's (a few ulps); a discrete mismatch on these inputs would be a bug unless the restatement shows the decision within a
few ulps of its bound.  The brute-force restatement is too slow beyond ~2 x 10^4 atoms, so the parity comparison stops there; the 10^5-atom
run checks completion and bit-identical repeats only."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import sc_restatement as R
import synth
from test_sc_host import hand_cases

pytestmark = pytest.mark.gpu
DATA = Path(__file__).resolve().parent / "data"


@pytest.fixture(scope="module")
def scr(tmp_path_factory):
    return R.compile(tmp_path_factory.mktemp("scr"))


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


def two_halves(n_atoms: int, gap: float = 0.6) -> dict:
    """The S2 ball of tests/synth.py cut at its middle plane: the lower half is molecule 0, the upper half (moved up by `gap`) molecule 1."""
    rec = synth.gen_s2(n_atoms)
    z = rec["z"].copy()
    mid = np.median(z)
    mol = (z > mid).astype(np.uint8)
    z[mol == 1] += gap
    cache = {}
    r = np.array([cache.setdefault(k, aa.sc_radius(k[0].decode(), k[1].decode(), k[2].decode()) or 1.8)
                  for k in zip(rec["resn"], rec["name"], rec["element"])])
    return {"x": rec["x"], "y": rec["y"], "z": z, "r": r, "mol": mol}


def compare(ctx, want, got):
    for k in ("n_convex", "n_toroidal", "n_concave", "n_probes"):
        assert got[k] == want[k], k
    for s in range(2):
        w = want["dots"][s]
        g = aa.sc_dots(ctx, s)
        assert len(g["flags"]) == len(w["flags"]), s
        assert np.array_equal(g["flags"].astype(np.int64), w["flags"].astype(np.int64)), s
        for k in ("xyz", "normal", "area", "nn_dist", "score"):
            np.testing.assert_allclose(g[k], w[k], rtol=1e-9, atol=1e-12, err_msg=f"surface {s} {k}")
        assert got["surfaces"][s]["n_trimmed_dots"] == want["n_trimmed_dots"][s]
    for k in ("sc", "distance", "area"):
        assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), k


def run_both(ctx, L, inp, serial=None):
    want = R.run(L, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"], serial)
    got = aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"], serial)
    return want, got


@pytest.mark.parametrize("groups", ["H/L", "H/C", "H,L/C,G"])
def test_parity_6bft(ctx, scr, groups):
    s = aa.load_model(str(DATA / "6bft.pdb"))
    inp = R.structure_inputs(s, groups)
    want, got = run_both(ctx, scr, inp, inp["serial"])
    assert want["err"] == 0
    compare(ctx, want, got)
    # the structure-level call selects, assigns radii and runs the same thing
    full = aa.get_sc_results(s, groups)
    assert full["sc"] == got["sc"] and full["n_toroidal"] == got["n_toroidal"]


def test_parity_1ubq_split(ctx, scr, tmp_path):
    lines = []
    for l in (DATA / "1ubq.pdb").read_text().splitlines():
        if l.startswith(("ATOM", "HETATM")) and int(l[22:26]) > 38:
            l = l[:21] + "B" + l[22:]
        lines.append(l)
    f = tmp_path / "1ubq_ab.pdb"
    f.write_text("\n".join(lines) + "\n")
    s = aa.load_model(str(f))
    inp = R.structure_inputs(s, "A/B")
    want, got = run_both(ctx, scr, inp, inp["serial"])
    assert want["err"] == 0
    compare(ctx, want, got)


def test_parity_synthetic_interface(ctx, scr):
    inp = two_halves(20_000)
    want, got = run_both(ctx, scr, inp)
    assert want["err"] == 0
    compare(ctx, want, got)
    # exact nearest neighbour: some trimmed dots find their partner beyond the first shell of 1.5 A cells
    nn = np.concatenate([aa.sc_dots(ctx, s)["nn_dist"] for s in range(2)])
    assert nn.max() > 1.5


def test_nn_beyond_first_shell(ctx, scr):
    # the halves 2.5 A apart: thousands of trimmed dots find their nearest partner more than one 1.5 A cell away (exact shell search)
    inp = two_halves(3000, gap=2.5)
    want, got = run_both(ctx, scr, inp)
    assert want["err"] == 0
    compare(ctx, want, got)
    nn = np.concatenate([d["nn_dist"][d["flags"] & 8 != 0] for d in (aa.sc_dots(ctx, 0), aa.sc_dots(ctx, 1))])
    assert (nn > 1.5).sum() > 1000  # (a partner more than one cell edge away can lie in the second shell)


@pytest.mark.parametrize("name", list(hand_cases()))
def test_hand_cases(ctx, scr, name):
    xyz, r, mol = hand_cases()[name]
    inp = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "r": r, "mol": mol}
    want = R.run(scr, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"])
    if name in R.BRANCHES:  # the case reaches the quirk it is named after (the restatement counts its branches)
        assert want["branches"][name] >= 1
    if want["err"]:
        with pytest.raises(aa.ArpeggiaError, match=R.ERRORS[want["err"]]):
            aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"])
    else:
        compare(ctx, want, aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"]))


@pytest.mark.parametrize("groups,want", [("H/L", 0.714), ("H/C", 0.785), ("H,L/C,G", 0.745)])
def test_reference_pins(groups, want):
    assert abs(aa.sc(str(DATA / "6bft.pdb"), groups) - want) < 0.05


def test_no_interface_raises():
    with pytest.raises(RuntimeError, match="No molecular dots generated"):
        aa.sc(str(DATA / "6bft.pdb"), "H/B")


def test_repeat_is_bit_identical(ctx):
    s = aa.load_model(str(DATA / "6bft.pdb"))
    a = aa.get_sc_results(s, "H,L/C,G")
    d1 = [aa.sc_dots(aa.api._context(0), k) for k in range(2)]
    b = aa.get_sc_results(s, "H,L/C,G")
    d2 = [aa.sc_dots(aa.api._context(0), k) for k in range(2)]
    assert a == b
    for u, v in zip(d1, d2):
        for k in u:
            assert np.array_equal(u[k], v[k]), k


def test_large_raw_run_repeats(ctx):
    inp = two_halves(100_000)
    a = aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"])
    da = [aa.sc_dots(ctx, k) for k in range(2)]
    b = aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"])
    db = [aa.sc_dots(ctx, k) for k in range(2)]
    assert a == b and 0.0 < a["sc"] < 1.0
    for u, v in zip(da, db):
        for k in u:
            assert np.array_equal(u[k], v[k]), k
