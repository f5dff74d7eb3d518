"""Shape complementarity across the frames of an ensemble on the device (arp_sc_ensemble), against the project's own single-frame call
(arp_sc + arp_sc_dots + arp_sc_dot_atoms) on the same context, frame by frame.  The single-frame call is pinned to the sequential
restatement and the reference's values by tests/test_sc_gpu.py and tests/test_sc_edge_gpu.py.

The contract per frame (check_frame):
    every integer field of arp_sc_results equal; d_median, s_median, sc and distance equal as doubles;
    trimmed_area, d_mean, s_mean and area within 2 (k - 1) 2^-53 sum|term| -- k the trimmed dots of the surface, the terms those of the
    single-frame call's dots (for a mean: the terms divided by k; for the combined area: both surfaces' terms): two orders of summing
    the same k terms cannot differ by more;
    the device statistics equal arp_sc_dot_stats_host on the single-frame call's dots bit for bit, sums included.
Every single-frame result is computed once per module (single()) and left unchanged."""
from __future__ import annotations

import re

import numpy as np
import pytest

import arpeggia_amd as aa
import ens_sasa_common as ens
import sc_edge_cases as E
import sc_ens_cases as EC

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
INT_SURFACE = ("n_atoms", "n_buried_atoms", "n_far_atoms", "n_all_dots", "n_trimmed_dots")
INT_TOP = ("n_convex", "n_toroidal", "n_concave", "n_probes")
DATA = __import__("pathlib").Path(__file__).parent / "data"


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def automatic_passes():
    yield
    aa.debug_set("sc_ens_frames", 0)


_SINGLE = {}


def single(ctx, key, inp, st):
    """The single-frame call on one frame: (results dict | error text, dots of both surfaces with their owner atoms)."""
    if key not in _SINGLE:
        try:
            res = aa.sc_arrays(ctx, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"], inp.get("serial"), E.api_settings(st))
        except aa.ArpeggiaError as e:
            _SINGLE[key] = (str(e), None)
        else:
            dots = []
            for m in range(2):
                d = aa.sc_dots(ctx, m)
                d["atom"] = aa.sc_dot_atoms(ctx, m).copy()
                dots.append(d)
            _SINGLE[key] = (res, dots)
    return _SINGLE[key]


def run_ensemble(ctx, case, frames=None):
    xyz, r, mol, st = case
    return aa.sc_arrays_ensemble(ctx, xyz if frames is None else xyz[list(frames)], r, mol, None, E.api_settings(st))


def check_frame(got, want, dots):
    """One frame of an ensemble call (a record of SC_RESULTS_DTYPE) against the single-frame call's results and dots."""
    surf = [want["surfaces"][0], want["surfaces"][1], want["combined"]]
    tol_area, tol_d, tol_s = [], [], []
    for m in range(2):
        t = (dots[m]["flags"] & EC.TRIMMED) != 0
        k = int(t.sum())
        assert k == want["surfaces"][m]["n_trimmed_dots"]
        tol_area.append(2.0 * max(k - 1, 0) * U * np.abs(dots[m]["area"][t]).sum())
        tol_d.append(2.0 * max(k - 1, 0) * U * np.abs(dots[m]["nn_dist"][t]).sum() / max(k, 1))
        tol_s.append(2.0 * max(k - 1, 0) * U * np.abs(dots[m]["score"][t]).sum() / max(k, 1))
    k_all = sum(int(s["n_trimmed_dots"]) for s in surf[:2])
    for m, s in enumerate(surf):
        g = got["surface"][m] if m < 2 else got["combined"]
        for k in INT_SURFACE:
            assert int(g[k]) == s[k], (m, k)
        for k in ("d_median", "s_median"):
            assert float(g[k]) == s[k], (m, k, float(g[k]), s[k])
        if m < 2:
            bounds = {"trimmed_area": tol_area[m], "d_mean": tol_d[m], "s_mean": tol_s[m]}
        else:  # sums and midpoints of the two surfaces: their bounds, plus the rounding of the one operation on top
            terms = sum(np.abs(dots[q]["area"][(dots[q]["flags"] & EC.TRIMMED) != 0]).sum() for q in range(2))
            bounds = {"trimmed_area": 2.0 * max(k_all - 1, 0) * U * terms, "d_mean": (tol_d[0] + tol_d[1]) / 2 + U * abs(s["d_mean"]),
                      "s_mean": (tol_s[0] + tol_s[1]) / 2 + U * abs(s["s_mean"])}
        for k, b in bounds.items():
            assert abs(float(g[k]) - s[k]) <= b, (m, k, float(g[k]), s[k], b)
    for k in INT_TOP:
        assert int(got[k]) == want[k], k
    assert float(got["sc"]) == want["sc"] and float(got["distance"]) == want["distance"]
    assert abs(float(got["area"]) - want["area"]) <= bounds["trimmed_area"]
    # the device statistics are the host twin's on the same dots, bit for bit
    n0, n1 = len(dots[0]["flags"]), len(dots[1]["flags"])
    cat = lambda k: np.concatenate([dots[0][k], dots[1][k]])
    twin = aa.sc_dot_stats([0, n0, n0 + n1], cat("flags"), cat("area"), cat("nn_dist"), cat("score"), [1, 0])
    for m in range(2):
        for k in ("n_all_dots", "n_trimmed_dots", "trimmed_area", "d_mean", "d_median", "s_mean", "s_median"):
            assert got["surface"][m][k].tobytes() == twin[m][k].tobytes(), (m, k)


def check_case(ctx, name, case, out=None):
    out = run_ensemble(ctx, case) if out is None else out
    for f in range(len(case[0])):
        want, dots = single(ctx, (name, f), EC.frame(case, f), case[3])
        assert out["status"][f] == 0, (f, EC.STATUS[out["status"][f]])
        check_frame(out["results"][f], want, dots)
    return out


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("results", "status", "err_atoms", "frames_in_interface", "trimmed_dots"))


def membership(ctx, name, case, frames):
    """frames_in_interface and trimmed_dots as numpy builds them from the single-frame calls' dots."""
    n = len(case[1])
    fi, td = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    for f in frames:
        _, dots = single(ctx, (name, f), EC.frame(case, f), case[3])
        cnt = np.zeros(n, np.uint64)
        for m in range(2):
            cnt += np.bincount(dots[m]["atom"][(dots[m]["flags"] & EC.TRIMMED) != 0], minlength=n).astype(np.uint64)
        fi += (cnt > 0).astype(np.uint32)
        td += cnt
    return fi, td


# ---- 1, 2, 6: six frames
SIX = EC.six_frames()


def test_frames_are_independent_and_in_order(ctx):
    out = check_case(ctx, "six", SIX)
    assert out["results"][0].tobytes() == out["results"][5].tobytes()
    assert len({out["results"][f].tobytes() for f in range(5)}) == 5  # the five frames do differ
    assert same(out, run_ensemble(ctx, SIX))  # two calls, the same bytes
    perm = [4, 2, 5, 0, 3, 1]
    moved = run_ensemble(ctx, SIX, perm)
    for k, f in enumerate(perm):
        assert moved["results"][k].tobytes() == out["results"][f].tobytes(), (k, f)
    for k in ("frames_in_interface", "trimmed_dots"):
        assert np.array_equal(moved[k], out[k])


def test_pass_edges(ctx):
    outs = []
    for b in (1, 2, 4, 6, 0):
        aa.debug_set("sc_ens_frames", b)
        outs.append(run_ensemble(ctx, SIX))
    for o in outs[1:]:
        assert same(o, outs[0])
    fi, td = membership(ctx, "six", SIX, range(6))
    assert np.array_equal(outs[0]["frames_in_interface"], fi) and np.array_equal(outs[0]["trimmed_dots"], td)


def test_per_atom_columns(ctx):
    out = run_ensemble(ctx, SIX, range(3))
    fi, td = membership(ctx, "six", SIX, range(3))
    assert fi.max() == 3 and 0 < (fi > 0).sum() < len(fi) and (td >= fi).all()
    assert np.array_equal(out["frames_in_interface"], fi) and np.array_equal(out["trimmed_dots"], td)
    assert out["frames_in_interface"].dtype == np.uint32 and out["trimmed_dots"].dtype == np.uint64


# ---- 3: failing frames inside a pass
def test_failing_frames_inside_a_pass(ctx):
    case, pair = EC.failing_frames()
    aa.debug_set("sc_ens_frames", 3)
    out = run_ensemble(ctx, case)  # (ARP_OK: a frame's physics is not a call failure)
    assert [EC.STATUS[k] for k in out["status"]] == ["ok", "no_dots", "ok", "coincident", "ok"]
    good = [0, 2, 4]
    for f in good:
        want, dots = single(ctx, ("fail", f), EC.frame(case, f), case[3])
        check_frame(out["results"][f], want, dots)
    alone = run_ensemble(ctx, case, good)  # the good frames without the failing ones next to them: unchanged
    for k, f in enumerate(good):
        assert alone["results"][k].tobytes() == out["results"][f].tobytes()
    for k in ("frames_in_interface", "trimmed_dots"):
        assert np.array_equal(alone[k], out[k])  # the per-atom columns count the good frames only
    fi, td = membership(ctx, "fail", case, good)
    assert np.array_equal(out["frames_in_interface"], fi) and np.array_equal(out["trimmed_dots"], td)
    # the failed frames: the single-frame call's error and what it leaves in *out
    n_atoms = [int((case[2] == m).sum()) for m in range(2)]
    msg, _ = single(ctx, ("fail", 1), EC.frame(case, 1), case[3])
    assert isinstance(msg, str) and "No molecular dots generated" in msg
    r = out["results"][1]
    assert [int(r["surface"][m]["n_atoms"]) for m in range(2)] == n_atoms
    assert all(int(r["surface"][m]["n_far_atoms"]) == n_atoms[m] and r["surface"][m]["n_buried_atoms"] == 0 for m in range(2))
    assert not r["combined"].tobytes().strip(b"\0") and r["sc"] == 0.0 and r["n_probes"] == 0
    msg, _ = single(ctx, ("fail", 3), EC.frame(case, 3), case[3])
    named = re.fullmatch(r"Overlapping atoms detected: (\d+) == (\d+)", msg)
    assert named and tuple(int(g) for g in named.groups()) == pair
    assert tuple(out["err_atoms"][3]) == pair
    assert (out["err_atoms"][[0, 1, 2, 4]] == 0xFFFFFFFF).all()
    r = out["results"][3].copy()
    assert [int(r["surface"][m]["n_atoms"]) for m in range(2)] == n_atoms
    r["surface"]["n_atoms"] = 0
    assert not r.tobytes().strip(b"\0")  # the atom counts, and the rest zero


# ---- 4: a surface without trimmed dots
def test_surface_without_trimmed_dots(ctx):
    case = EC.no_trim_frame()
    want, dots = single(ctx, ("no_trim", 0), EC.frame(case, 0), case[3])
    assert min(s["n_all_dots"] for s in want["surfaces"]) > 0 and want["surfaces"][0]["n_trimmed_dots"] == 0 < want["surfaces"][1]["n_trimmed_dots"]
    out = check_case(ctx, "no_trim", case)
    r = out["results"][0]
    assert out["status"][0] == 0 and r["sc"] == 0.0 and r["distance"] == 0.0
    for m in range(2):
        assert not any(float(r["surface"][m][k]) for k in ("d_mean", "d_median", "s_mean", "s_median"))
    assert r["surface"][1]["trimmed_area"] > 0.0 and r["area"] == r["surface"][1]["trimmed_area"]
    # its one trimmed dot counts in the per-atom columns, as in the dots of the single-frame call
    fi, td = membership(ctx, "no_trim", case, [0])
    assert td.sum() == want["surfaces"][1]["n_trimmed_dots"] and np.array_equal(out["trimmed_dots"], td) and np.array_equal(out["frames_in_interface"], fi)


# ---- 5: latitudes past one wave, a third scan level inside a slab
@pytest.mark.parametrize("name", ["contact_density", "contact_radii", "concave_d190"])
def test_wave_kernels_across_frames(ctx, name):
    kind, _, key = name.partition("_")
    cases = E.lat_chunks_contact() if kind == "contact" else {k.split("_")[1]: v for k, v in E.lat_chunks_concave().items()}
    check_case(ctx, name, EC.shifted_pair(cases[key]))


def test_wide_slab_next_to_a_compact_frame(ctx):
    case = EC.wide_and_compact()
    out = check_case(ctx, "wide", case)
    assert out["results"][0]["n_probes"] == out["results"][1]["n_probes"] > 0  # (the far atom changes no dot in either frame)


# ---- 7: the selection kernel at its edges
STATS = EC.stats_cases()


@pytest.mark.parametrize("name", list(STATS))
def test_dot_stats_kernel(name):
    case = STATS[name]
    dev, host, ref = aa.sc_dot_stats(*case, device=0), aa.sc_dot_stats(*case), EC.stats_reference(*case)
    assert dev.tobytes() == host.tobytes()
    for k in ("d_median", "s_median"):
        assert np.array_equal(dev[k], ref[k]), k  # np.partition's element k // 2
    for k in ("n_all_dots", "n_trimmed_dots"):
        assert np.array_equal(dev[k], ref[k]), k
    if name == "median_zero":
        assert dev["s_median"][0] == 0.0 and np.signbit(dev["s_median"][0])
    if name == "other_empty":
        assert dev["n_trimmed_dots"][0] > 0 and not any(dev[k].any() for k in ("d_mean", "d_median", "s_mean", "s_median"))


# ---- 8: the structure level
@pytest.fixture(scope="module")
def bft():
    return aa.load_model(str(DATA / "6bft.pdb"))


def structure_single(ctx, bft):
    """get_sc_results on the module's context, with the dots: through sc_arrays on the selection (the same call underneath)."""
    atoms, mol = aa.sc_select(bft, "H/L")
    xyz = ens.topology_xyz(bft)[atoms]
    names, resn, elem = (bft.strings(k)[atoms] for k in ("atomn", "resn", "element"))
    r = np.array([aa.sc_radius(b.decode(), a.decode(), e.decode()) for a, b, e in zip(names, resn, elem)])
    inp = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "r": r, "mol": mol, "serial": bft.ints("atomi")[atoms].astype(np.int64)}
    return single(ctx, ("6bft", 0), inp, dict(E.DEFAULTS)), atoms


def test_structure_level(ctx, bft, tmp_path):
    (want, dots), atoms = structure_single(ctx, bft)
    direct = aa.get_sc_results(bft, "H/L")
    assert direct == want  # the arrays above are what arp_structure_sc works on
    out = ctx.sc_ensemble(bft, None, "H/L")
    assert out["n_frames"] == 1 and np.array_equal(out["atoms"], atoms) and out["status"][0] == 0
    check_frame(out["results"][0], want, dots)
    base = ens.topology_xyz(bft)
    frames = np.stack([base, base + np.random.default_rng(1).normal(0.0, 0.05, base.shape), base + np.random.default_rng(2).normal(0.0, 0.05, base.shape)])
    out3 = ctx.sc_ensemble(bft, frames, "H/L")
    assert out3["n_frames"] == 3 and out3["results"][0].tobytes() == out["results"][0].tobytes()
    assert out3["results"][1]["sc"] != out3["results"][0]["sc"]
    ft, at = aa.get_sc_ensemble(bft, frames, "H/L")
    ft = ft if hasattr(ft, "column_names") else ft.to_arrow()
    at = at if hasattr(at, "column_names") else at.to_arrow()
    assert ft.column_names == aa.SC_FRAME_COLUMNS and at.column_names == aa.SC_ENSEMBLE_COLUMNS
    assert ft.num_rows == 3 and at.num_rows == len(atoms)
    assert ft.column("status").to_pylist() == ["ok"] * 3 and ft.column("sc").to_pylist()[0] == want["sc"]
    assert at.column("n_frames").to_pylist() == [3] * len(atoms)
    assert np.array_equal(np.array(at.column("occupancy").to_pylist()), out3["frames_in_interface"] / 3.0)
    assert np.array_equal(np.array(at.column("mean_trimmed_dots").to_pylist()), out3["trimmed_dots"] / 3.0)
    # the command writes the table of the file's models
    from arpeggia_amd.__main__ import main
    import pyarrow.csv as pacsv

    assert main(["sc-ensemble", "-i", str(DATA / "6bft.pdb"), "-g", "H/L", "-o", str(tmp_path), "--atoms"]) == 0
    csv = pacsv.read_csv(str(tmp_path / "sc_ensemble.csv"))
    ft1, at1 = aa.sc_ensemble(str(DATA / "6bft.pdb"), "H/L")
    ft1 = ft1 if hasattr(ft1, "column_names") else ft1.to_arrow()
    assert csv.column_names == aa.SC_FRAME_COLUMNS and csv.num_rows == 1
    assert csv.column("sc").to_pylist() == ft1.column("sc").to_pylist() == [want["sc"]]
    assert csv.column("n_trimmed_dots_1").to_pylist() == [want["surfaces"][0]["n_trimmed_dots"]]
    assert pacsv.read_csv(str(tmp_path / "sc_ensemble_atoms.csv")).column_names == aa.SC_ENSEMBLE_COLUMNS
