"""Shape complementarity across frames, the part that needs no device: arp_sc_dot_stats_host against numpy and against a Python restatement
of its summation order (sc_ens_cases.stats_reference); every input error of the ensemble entry points through their ctx = None mode; the
column lists; and, with the sequential restatement (tests/sc_restatement.c), that the cases of tests/sc_ens_cases.py which are named for a
path reach it: the failing frames fail as named, the frame without trimmed dots has dots on both surfaces and no trimmed dot on one, the
latitude and wide-box frames keep what tests/test_sc_edge_host.py shows for their first frame."""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import ens_sasa_common as ens
import sc_edge_cases as E
import sc_ens_cases as EC
import sc_restatement as R
import synth
from arpeggia_amd import _lib
from arpeggia_amd.api import _sc_ensemble, _topology_atoms

DATA = __import__("pathlib").Path(__file__).parent / "data"


@pytest.fixture(scope="module")
def scr(tmp_path_factory):
    return R.compile(tmp_path_factory.mktemp("scr"))


@pytest.fixture(scope="module")
def bft():
    return aa.load_model(str(DATA / "6bft.pdb"))


def restated(scr, case, f):
    inp = EC.frame(case, f)
    return R.run(scr, inp["x"], inp["y"], inp["z"], inp["r"], inp["mol"], None, **case[3])


def refused(fn, *args, status=_lib.ARP_ERR_BAD_INPUT, match=None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


# ---- the statistics twin on the host
STATS = EC.stats_cases()


@pytest.mark.parametrize("name", list(STATS))
def test_dot_stats_host_against_numpy(name):
    case = STATS[name]
    got, want = aa.sc_dot_stats(*case), EC.stats_reference(*case)
    for k in ("n_all_dots", "n_trimmed_dots"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("n_atoms", "n_buried_atoms", "n_far_atoms"):
        assert not got[k].any()
    # the medians are elements of the input: equal as doubles (a zero may differ in sign from numpy's pick, not in value)
    for k in ("d_median", "s_median"):
        assert np.array_equal(got[k], want[k]), k
    # the sums follow the stated order: bit for bit against its Python restatement
    for k in ("trimmed_area", "d_mean", "s_mean"):
        assert got[k].tobytes() == want[k].tobytes(), k


def test_dot_stats_host_rules():
    seg, fl, a, d, s, other = STATS["other_empty"]
    got = aa.sc_dot_stats(seg, fl, a, d, s, other)
    assert got["n_trimmed_dots"][0] > 0 and got["n_trimmed_dots"][1] == 0
    assert got["trimmed_area"][0] > 0.0  # the area is kept, the neighbour statistics are zero on both sides
    for k in ("d_mean", "d_median", "s_mean", "s_median"):
        assert not got[k].any(), k
    seg, fl, a, d, s, other = STATS["median_zero"]
    got = aa.sc_dot_stats(seg, fl, a, d, s, other)
    assert got["s_median"][0] == 0.0 and np.signbit(got["s_median"][0])  # -0.0 is element k / 2 and keeps its sign
    # an even count takes the upper of the two middle elements, no average
    got = aa.sc_dot_stats([0, 2, 3], [8, 8, 8], [1.0, 1.0, 1.0], [1.0, 2.0, 5.0], [0.1, 0.3, 0.2], [1, 0])
    assert got["d_median"][0] == 2.0 and got["s_median"][0] == 0.3 and got["d_mean"][0] == 1.5
    # malformed segments
    refused(aa.sc_dot_stats, [0, 2, 1, 3], [8, 8, 8], [1.0] * 3, [1.0] * 3, [0.0] * 3, [0, 0, 0], match="seg_start must not decrease")
    refused(aa.sc_dot_stats, [0, 3], [8, 8, 8], [1.0] * 3, [1.0] * 3, [0.0] * 3, [1], match="names no segment")
    refused(aa.sc_dot_stats, [0, 2], [8, 8, 8], [1.0] * 3, [1.0] * 3, [0.0] * 3, [0], match="seg_start")


def test_sum_order_depends_on_the_segment_alone():
    # the same segment alone, and as segment 3 of 5 behind others: the same bytes
    rng = np.random.default_rng(5)
    n = 777
    fl = np.where(rng.random(n) < 0.5, 8, 0)
    a, d, s = rng.random(n), rng.random(n), rng.normal(size=n)
    alone = aa.sc_dot_stats([0, n], fl, a, d, s, [0])
    pre = 1234
    cat = lambda v, fill: np.concatenate([np.full(pre, fill, dtype=np.asarray(v).dtype), v, np.full(99, fill, dtype=np.asarray(v).dtype)])
    among = aa.sc_dot_stats([0, 1000, pre, pre, pre + n, pre + n + 99], cat(fl, 8), cat(a, 0.3), cat(d, 0.7), cat(s, 0.1), [0, 1, 2, 3, 4])
    assert alone[0].tobytes() == among[3].tobytes()


# ---- input errors, through the ctx = None mode
def test_structure_input_errors(bft):
    n = _topology_atoms(bft)
    xyz0 = ens.topology_xyz(bft)
    ok = _sc_ensemble(None, bft, None, "H/L")
    assert ok["n_frames"] == 1 and len(ok["atoms"]) == len(ok["molecule"]) > 0
    atoms, mol = aa.sc_select(bft, "H/L")
    assert np.array_equal(ok["atoms"], atoms) and np.array_equal(ok["molecule"], mol)
    frames = np.repeat(xyz0[None], 5, 0)
    assert _sc_ensemble(None, bft, frames, "H/L")["n_frames"] == 5
    refused(_sc_ensemble, None, bft, frames[:, :-1], "H/L", match=f"frames must have shape [F, {n}, 3]")
    refused(_sc_ensemble, None, bft, frames[:0], "H/L", match="at least one frame")
    bad = frames.copy()
    bad[3, atoms[10], 1] = np.nan
    bad[4, atoms[2], 0] = np.inf
    refused(_sc_ensemble, None, bft, bad, "H/L", match=f"non-finite coordinate in frame 3, atom {atoms[10]}")
    bad = frames.copy()
    bad[2, np.setdiff1d(np.arange(n), atoms)[0]] = np.nan  # an atom outside the selection is not read
    assert _sc_ensemble(None, bft, bad, "H/L")["n_frames"] == 5
    refused(_sc_ensemble, None, bft, frames, "H,L", status=_lib.ARP_ERR_BAD_GROUPS, match="Invalid chain groups format")
    every = ",".join(sorted(set(c.decode() for c in bft.strings("chain"))))
    refused(_sc_ensemble, None, bft, frames, every + "/", status=_lib.ARP_ERR_EMPTY_GROUPS)
    refused(aa.get_sc_ensemble, bft, frames, "H,L", status=_lib.ARP_ERR_BAD_GROUPS)  # an input error comes ahead of a missing device


def test_missing_radius():
    # An atom with no Lawrence & Colman entry and no van der Waals class has radius 0 (arp_sc_radius); the raw call refuses it by atom.  At
    # the structure level the same atom never arrives: both ingest paths refuse an element without radii, so arp_structure_sc_ensemble's own
    # message (arp_structure_sc's) is a second line behind them.
    assert aa.sc_radius("UNX", "XQ9", "FE") == 0.0
    xyz, r, mol, _ = EC.six_frames(60)
    r[17] = aa.sc_radius("UNX", "XQ9", "FE")
    refused(aa.sc_arrays_ensemble, None, xyz, r, mol, match="atom 17: the radius must be finite and > 0")
    rec = {k: v.copy() for k, v in synth.gen_s2(60).items()}
    rec["chain"][30:] = b"B"
    rec["element"][5], rec["name"][5] = b"FE", b"FE1"
    with pytest.raises(aa.ArpeggiaError, match="element 'FE' has no radii"):
        aa.Structure.from_records(rec)


def test_raw_input_errors():
    case = EC.six_frames(60)
    xyz, r, mol, _ = case
    assert aa.sc_arrays_ensemble(None, xyz, r, mol)["n_frames"] == 6  # the checks only
    refused(aa.sc_arrays_ensemble, None, xyz[:, :-1], r, mol, match="xyz must have shape")
    refused(aa.sc_arrays_ensemble, None, xyz[:0], r, mol, match="at least one frame")
    bad = xyz.copy()
    bad[3, 11, 2] = np.nan
    refused(aa.sc_arrays_ensemble, None, bad, r, mol, match="non-finite coordinate in frame 3, atom 11")
    for k, v in ((0, 0.0), (5, np.nan), (7, -1.0)):
        rr = r.copy()
        rr[k] = v
        refused(aa.sc_arrays_ensemble, None, xyz, rr, mol, match=f"atom {k}: the radius must be finite and > 0")
    refused(aa.sc_arrays_ensemble, None, xyz, r, np.where(np.arange(len(r)) == 3, 2, mol), match="molecule must be 0 or 1")
    refused(aa.sc_arrays_ensemble, None, xyz, r, np.ones_like(mol), match="No atoms for chain group 1")
    refused(aa.sc_arrays_ensemble, None, xyz, r, mol, np.zeros(len(r), np.int64), match="duplicate atom serial numbers")
    refused(aa.sc_arrays_ensemble, None, xyz, r, mol, None, {"dot_density": 0.0}, match="bad SC settings")
    assert _lib.lib.arp_sc_ensemble(None, 5, 2, None, None, None, None, None, None, None, None, None, None) == _lib.ARP_ERR_BAD_INPUT
    assert b"null argument" in _lib.lib.arp_last_error()
    with pytest.raises(aa.ArpeggiaError, match="sc_ens_frames"):
        aa.debug_set("sc_ens_frames", -1)
    aa.debug_set("sc_ens_frames", 0)


def test_column_lists():
    assert aa.SC_FRAME_COLUMNS[:5] == ["frame", "status", "sc", "distance", "area"]
    per = ["n_all_dots", "n_trimmed_dots", "trimmed_area", "d_median", "s_median", "d_mean", "s_mean"]
    assert aa.SC_FRAME_COLUMNS[5:19] == [f"{k}_{m}" for k in per for m in (1, 2)]
    assert aa.SC_FRAME_COLUMNS[19:] == ["n_probes", "n_convex", "n_toroidal", "n_concave"]
    assert aa.SC_ENSEMBLE_COLUMNS == aa.DSASA_ENSEMBLE_COLUMNS[:7] + ["molecule", "n_frames", "occupancy", "mean_trimmed_dots"]
    assert aa.SC_FRAME_STATUS == list(EC.STATUS)
    assert aa.SC_RESULTS_DTYPE.itemsize == _lib.C.sizeof(_lib.arp_sc_results)
    # the frame table from arrays alone: a failed frame has nulls in the float columns, numbers in the integer ones
    res = np.zeros(2, aa.SC_RESULTS_DTYPE)
    res["sc"] = [0.7, 0.0]
    res["surface"]["n_all_dots"][1] = [5, 0]
    t = aa.sc_frame_table(res, [0, 1])
    t = t if hasattr(t, "column_names") else t.to_arrow()
    assert t.column_names == aa.SC_FRAME_COLUMNS
    rows = t.to_pylist()
    assert rows[0]["status"] == "ok" and rows[0]["sc"] == 0.7 and rows[1]["status"] == "no_dots"
    assert rows[1]["sc"] is None and rows[1]["d_mean_2"] is None and rows[1]["n_all_dots_1"] == 5 and rows[1]["n_probes"] == 0


# ---- the cases reach what they are named for
def test_failing_frames_fail_as_named(scr):
    case, (i, j) = EC.failing_frames()
    xyz, r, mol, st = case
    assert mol[i] == mol[j] == 0 and i < j and np.array_equal(xyz[3, i], xyz[3, j])
    for f, name in ((0, ""), (1, "No molecular dots generated"), (3, "Overlapping atoms detected")):
        out = restated(scr, case, f)
        if name:
            assert name.lower() in R.ERRORS[out["err"]].lower(), (f, R.ERRORS[out["err"]])
        else:
            assert out["err"] == 0 and min(out["n_trimmed_dots"]) > 0


def test_no_trim_frame_reach(scr):
    out = restated(scr, EC.no_trim_frame(), 0)
    assert out["err"] == 0 and min(out["n_all_dots"]) > 0
    assert out["n_trimmed_dots"][0] == 0 and out["n_trimmed_dots"][1] > 0, out["n_trimmed_dots"]
    assert out["sc"] == 0.0 and out["distance"] == 0.0  # calc_neighbor_distance returns early on both sides


def test_shifted_frames_keep_their_reach(scr):
    # frame 1 of the latitude cases (frame 0 moved 0.5 A): as many latitudes as frame 0, whose reach tests/test_sc_edge_host.py asserts
    for name, single in list(E.lat_chunks_contact().items())[:1] + list(E.lat_chunks_concave().items())[1:2]:
        case = EC.shifted_pair(single)
        a, b = restated(scr, case, 0), restated(scr, case, 1)
        assert a["err"] == b["err"] == 0
        assert max(b["reach"]["max_lat_contact"], b["reach"]["max_lat_probe"]) > 64
        assert (a["reach"]["max_lat_contact"], a["reach"]["max_lat_probe"]) == (b["reach"]["max_lat_contact"], b["reach"]["max_lat_probe"])


def test_wide_and_compact_cell_counts():
    xyz, r, mol, st = case = EC.wide_and_compact()
    for edge in (E.TRIM_EDGE, E.open_edge(st)):
        dims, capped = E.cell_dims(EC.frame(case, 0), st, edge)
        assert not capped and dims[0] * dims[1] * dims[2] + 1 > 1024 * 1024  # a third scan level inside one slab
        dims, capped = E.cell_dims(EC.frame(case, 1), st, edge)
        assert not capped and dims[0] * dims[1] * dims[2] < 1024 * 1024
