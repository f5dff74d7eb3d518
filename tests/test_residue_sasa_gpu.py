"""Residue- and chain-level SASA, relative SASA and the segment sums behind them on the device.

Expected values never come from the new path: per-atom SASA is the array call aa.atom_sasa with radii from the table typed into
tests/residue_sasa_common.py, the sums are sequential f64 loops in Python, the grouping is Python.  Everything is compared for equality: the
per-atom values are exact (integer counts) and the sums have a fixed order.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import ens_sasa_common as ec
import residue_sasa_common as rc
from residue_sasa_common import atom_values, expected_levels

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


# ---- 7. arp_segment_sum against the sequential loop ------------------------------------------------------------------------------------------
# Order must show after the f32 rounding.  PATTERN in list order: 2^24 + 1 is exact in f64, every following 2^-30 is a quarter of an f64 ulp
# and is lost, and 2^24 + 1 ties to the even 2^24 in f32.  With the small items first (reversed, or summed pairwise) they add up to 2^-27 and
# the sum lies above the tie: 2^24 + 2.  MIRROR is the same ten items the other way round: in list order 2^24 + 2, reversed 2^24.
PATTERN = np.array([2.0 ** 24, 1.0] + [2.0 ** -30] * 8, np.float32)
MIRROR = PATTERN[::-1].copy()
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 129, 1000, 20000)


def _with(length, pos, pat):
    seq = np.zeros(length, np.float32)
    seq[pos:pos + len(pat)] = pat
    return seq


def build_segments():
    """[(name, kind, values in list order, layout)]: kind random / pattern / mirror; layout says how the segment's items lie in a row."""
    rng = np.random.default_rng(7)
    segs = []
    for L in LENGTHS[:-1]:
        segs.append((f"random{L}", "random", rng.uniform(0.0, 30.0, L).astype(np.float32), "contiguous"))
    for L in (63, 64, 65, 127, 129, 1000):
        spots = [("head", 0), ("tail", L - 10)] + ([("edge64", 60)] if L > 70 else []) + ([("edge576", 571)] if L > 600 else [])
        group = []
        for where, pos in spots:
            # (a forward pattern in the last n % 8 items of a segment is what numpy's pairwise sum adds last, one by one: there np.sum follows
            # the list order and shows nothing -- lengths 63 and 127 take the mirror image alone at the tail)
            if not (where == "tail" and L % 8 == 7):
                group.append((f"pattern{L}@{where}", "pattern", _with(L, pos, PATTERN)))
            group.append((f"mirror{L}@{where}", "mirror", _with(L, pos, MIRROR)))
        pairs = (len(group) - 2) // 2  # the first two lie contiguous and reversed, the rest interleaved two by two (an odd one out: reversed)
        for k, (name, kind, seq) in enumerate(group):
            lay = "contiguous" if k == 0 else "interleaved" if 2 <= k < 2 + 2 * pairs else "reversed"
            segs.append((name, kind, seq, lay))
    segs.append(("pattern20000@edge12800", "pattern", _with(20000, 12796, PATTERN), "contiguous"))
    # two segments that share one item, the 2^24 at the head of both
    segs.append(("pattern65@shared-a", "pattern", _with(65, 0, PATTERN), "contiguous"))
    segs.append(("pattern65@shared-b", "pattern", _with(65, 0, PATTERN), "shares-first-with-previous"))
    return segs


def lay_out(segs, rows, seed):
    """values [rows, m], seg_start, seg_item.  Pattern segments hold the same items in every row, random ones are drawn per row."""
    start, items, cursor, k = [0], [], 0, 0
    while k < len(segs):
        L, lay = len(segs[k][2]), segs[k][3]
        if lay == "interleaved" and k + 1 < len(segs) and segs[k + 1][3] == "interleaved" and len(segs[k + 1][2]) == L:
            idx = np.arange(cursor, cursor + 2 * L)
            items += [idx[0::2], idx[1::2]]
            cursor += 2 * L
            k += 2
            continue
        idx = np.arange(cursor, cursor + L)
        cursor += L
        if lay == "reversed":
            idx = idx[::-1]
        if lay == "shares-first-with-previous":
            idx = idx.copy()
            idx[0] = items[-1][0]
        items.append(idx)
        k += 1
    m = cursor + 37
    m += 1 if m % 64 == 0 else 0
    rng = np.random.default_rng(seed)
    values = rng.uniform(0.0, 30.0, (rows, m)).astype(np.float32)
    for r in range(rows):
        for (name, kind, seq, lay), idx in zip(segs, items):
            if kind != "random" or r == 0:
                values[r, idx] = seq
    for idx in items:
        start.append(start[-1] + len(idx))
    item = np.concatenate(items).astype(np.uint32)
    return values, np.array(start, np.uint32), item


@pytest.fixture(scope="module")
def seg_case():
    segs = build_segments()
    out = {}
    for rows in (1, 5):
        values, start, item = lay_out(segs, rows, seed=rows)
        out[rows] = (values, start, item, rc.segment_sums(values, start, item))
    return segs, out


def test_segment_sum_cases_show_the_order(seg_case):
    """The test may not hide a wrong order: on the CPU, every pattern segment's sequential sum differs from the reversed-order sum and from
    np.sum (pairwise), and every mirror segment's from the reversed-order sum.  A mirror image cannot differ from a pairwise sum, whatever it
    is built from: its small items come first, so the list order keeps them -- as any pairwise tree does -- and a sum of non-negative items
    has only the two f32 neighbours of the tie to land on.  The mirror images are there for a kernel that walks a segment from its end."""
    segs, out = seg_case
    values, start, item, want = out[1]
    kinds = [s[1] for s in segs]
    assert sorted({len(s[2]) for s in segs}) == sorted(LENGTHS) and kinds.count("pattern") >= 15 and kinds.count("mirror") >= 15
    assert {s[3] for s in segs} == {"contiguous", "reversed", "interleaved", "shares-first-with-previous"}
    assert values.shape[1] % 64 != 0
    shown = 0
    for k, (name, kind, seq, lay) in enumerate(segs):
        listed = values[0, item[start[k]:start[k + 1]].astype(np.int64)]
        assert np.array_equal(listed, seq), name  # the layout put the items where the list says
        if kind == "random":
            continue
        forward, backward, pairwise = rc.seq_sum(seq), rc.seq_sum(seq[::-1]), np.float32(np.sum(seq.astype(np.float64)))
        assert forward == want[0, k] == np.float32(2.0 ** 24 if kind == "pattern" else 2.0 ** 24 + 2.0), name
        assert forward != backward, name
        if kind == "pattern":
            assert forward != pairwise, name
        shown += 1
    assert shown == kinds.count("pattern") + kinds.count("mirror")  # no constructed segment is exempt
    # a pattern sits at the head, across a 64-item boundary and at the tail of short and of long segments
    names = " ".join(s[0] for s in segs)
    for tag in ("pattern64@head", "pattern64@tail", "pattern129@edge64", "pattern129@tail", "pattern1000@head", "pattern1000@edge576", "pattern1000@tail",
                "mirror63@tail", "mirror127@tail", "mirror127@edge64", "pattern20000@edge12800"):
        assert tag in names, tag


@pytest.mark.parametrize("rows", [1, 5])
def test_segment_sum_is_the_sequential_chain(ctx, seg_case, rows):
    segs, out = seg_case
    values, start, item, want = out[rows]
    got = aa.segment_sum(ctx, values, start, item)
    assert got.dtype == np.float32 and got.shape == (rows, len(segs))
    bad = [(r, segs[k][0], float(got[r, k]), float(want[r, k])) for r, k in zip(*np.nonzero(got.view(np.uint32) != want.view(np.uint32)))]
    assert not bad, bad[:10]
    assert got[0, 0] == 0.0 and len(segs[0][2]) == 0  # an empty segment
    again = aa.segment_sum(ctx, values, start, item)
    assert again.tobytes() == got.tobytes()


def test_segment_sum_of_nothing(ctx):
    assert aa.segment_sum(ctx, np.zeros((0, 5), np.float32), [0, 1], [0]).shape == (0, 1)
    assert aa.segment_sum(ctx, np.ones((2, 5), np.float32), [0], []).shape == (2, 0)
    assert np.array_equal(aa.segment_sum(ctx, np.ones((2, 5), np.float32), [0, 0, 5, 5], [4, 3, 2, 1, 0]), [[0.0, 5.0, 0.0]] * 2)


# ---- 8. the single-structure levels ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_points", [1, 64, 100])
@pytest.mark.parametrize("radii", ["protor", "vdw"])
@pytest.mark.parametrize("which,chains", [("ubq", ""), ("bft", ""), ("bft", "H,L"), ("ubq", "H,L")])
def test_levels_equal_the_loop_over_atom_sasa(ctx, request, which, chains, radii, n_points):
    s = request.getfixturevalue(which)
    sel = rc.select_1_to_4(s, chains)
    res_t = rc.columns(aa.get_residue_sasa(s, 1.4, n_points, 0, chains, radii))
    chn_t = rc.columns(aa.get_chain_sasa(s, 1.4, n_points, 0, chains, radii))
    rel_t = rc.columns(aa.get_relative_sasa(s, 1.4, n_points, 0, chains, radii))
    assert list(res_t) == aa.RESIDUE_SASA_COLUMNS and list(chn_t) == aa.CHAIN_SASA_COLUMNS and list(rel_t) == aa.RELATIVE_SASA_COLUMNS
    if which == "ubq" and chains:  # 1ubq has no chain H or L: an empty selection
        assert len(sel) == 0 and len(res_t["sasa"]) == 0 and len(chn_t["sasa"]) == 0 and len(rel_t["sasa"]) == 0
        return
    values = atom_values(ctx, s, sel, radii, n_points)
    res, res_sum, chn, chn_sum = expected_levels(s, sel, values)
    # row identity and order
    assert list(zip(res_t["chain"], res_t["resn"], res_t["resi"], res_t["insertion"])) == [k for k, _ in res]
    assert chn_t["chain"] == [c for c, _ in chn] == sorted(chn_t["chain"])
    keys = [(c.encode(), i, n.encode()) for c, i, n in zip(res_t["chain"], res_t["resi"], res_t["insertion"])]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    if chains:
        assert set(chn_t["chain"]) == set(chains.split(","))
    # the values, exactly
    assert np.array_equal(np.array(res_t["sasa"], np.float32), res_sum)
    assert np.array_equal(np.array(chn_t["sasa"], np.float32), chn_sum)
    assert res_t["is_polar"] == [k[1] in rc.POLAR for k, _ in res]
    # relative SASA: one f32 division, null without a MaxASA
    assert rel_t["sasa"] == res_t["sasa"] and rel_t["is_polar"] == res_t["is_polar"]
    for (key, _), v, rel in zip(res, res_sum, rel_t["relative_sasa"]):
        mx = rc.MAX_ASA.get(key[1].upper())
        if mx is None:
            assert rel is None, key
        else:
            assert np.float32(rel) == np.float32(v) / np.float32(mx), key
    if which == "ubq":
        assert len(res_t["sasa"]) == 76 and chn_t["chain"] == ["A"] and res_t["resi"] == list(range(1, 77))
    else:
        assert len(res_t["sasa"]) > 300 and len(chn_t["chain"]) == (2 if chains else len(set(s.strings("chain")[sel].tolist())))


def test_1ubq_totals_and_relative_sasa(ctx, ubq, ubq_path):
    chain_total = rc.columns(aa.get_chain_sasa(ubq))["sasa"]
    assert len(chain_total) == 1
    print("1ubq chain total, ProtOr radii:", chain_total[0])
    assert abs(chain_total[0] - 4813.0) <= 100.0  # sasa.rs test_sasa_regression_ubiquitin
    assert np.float32(chain_total[0]) == np.float32(rc.protor_total_of_1ubq(ubq))  # the CPU restatement of tests/test_residue_sasa_host.py, exactly
    res_total = float(np.sum(np.array(rc.columns(aa.get_residue_sasa(ubq))["sasa"], np.float64)))
    atom_total = float(np.sum(np.array(rc.columns(aa.get_atom_sasa(ubq))["sasa"], np.float64)))
    assert 0.9 < res_total / atom_total < 1.1  # sasa.rs test_sasa_levels_consistent
    rsa = np.array(rc.columns(aa.relative_sasa(ubq_path))["relative_sasa"], np.float64)
    assert len(rsa) == 76 and not np.isnan(rsa).any()
    assert (rsa >= 0.0).all() and (rsa <= 1.5).mean() > 0.95  # sasa.rs test_relative_sasa_values_reasonable
    print("1ubq RSA: max", rsa.max(), "share <= 1.0", (rsa <= 1.0).mean())


def test_sasa_with_a_table_name_offers_every_level(ubq_path, ubq):
    res = rc.columns(aa.sasa(ubq_path, level="residue", radii="protor"))
    assert res == rc.columns(aa.get_residue_sasa(ubq))
    assert rc.columns(aa.sasa(ubq_path, level="chain", radii="vdw")) == rc.columns(aa.get_chain_sasa(ubq, radii="vdw"))
    # the atom level: radii None and "vdw" are the same bytes, "protor" is another table
    a0, a1, a2 = (rc.columns(aa.sasa(ubq_path, radii=r)) for r in (None, "vdw", "protor"))
    assert a0 == a1 and a0["sasa"] != a2["sasa"] and a0["atomi"] == a2["atomi"]
    sel = rc.select_1_to_4(ubq)
    # (1ubq's serial numbers ascend: the rows are in selection order)
    want = atom_values(aa.api._context(0), ubq, sel, "protor", 100)
    assert np.array_equal(np.array(a2["sasa"], np.float32), want)


# ---- 9. dSASA with a named table -------------------------------------------------------------------------------------------------------------
def test_dsasa_with_protor_radii(ctx, bft):
    d = aa.get_dsasa(bft, "C/H,L", radii="protor")
    print("6bft C/H,L dSASA, ProtOr radii:", d)
    assert abs(d - 1650.0) <= 50.0  # sasa.rs test_get_dsasa_interface_value
    a, b = aa.get_dsasa(bft, "A,B,C/G,H,L", radii="protor"), aa.get_dsasa(bft, "G,H,L/A,B,C", radii="protor")
    assert a > 0 and abs(a - b) < 1.0
    # restated from the array call: complex, group 1 and group 2 as three runs, each total an f64 sum rounded to f32, then f32 arithmetic
    for radii in ("protor", "vdw"):
        totals = []
        for chains in ("C,H,L", "C", "H,L"):
            sel = rc.select_1_to_4(bft, chains)
            totals.append(np.float32(np.cumsum(atom_values(ctx, bft, sel, radii, 100).astype(np.float64))[-1]))
        want = np.float32(np.float32(totals[1] + totals[2]) - totals[0])
        assert np.float32(aa.get_dsasa(bft, "C/H,L", radii=radii)) == want
        if radii == "vdw":
            assert np.float32(aa.get_dsasa(bft, "C/H,L")) == want  # radii None: the bytes of before
    with pytest.raises(ValueError):
        aa.get_dsasa(bft, "C/H,L", radii="chothia")


# ---- 10. the residue level across the frames of an ensemble ------------------------------------------------------------------------------------
RES_KEYS = ("mean_sasa", "std_sasa", "min_sasa", "max_sasa", "mean_relative_sasa", "chain_sasa", "residue_sasa", "is_polar", "relative_valid",
            "res_atoms", "chain_atoms")


def jittered(s, n_frames):
    base = ec.topology_xyz(s)
    return base[None] + np.random.default_rng(0).normal(scale=0.3, size=(n_frames,) + base.shape)


@pytest.mark.parametrize("which,F,chains", [("ubq", 8, ""), ("bft", 4, "H,L")])
def test_residue_ensemble(ctx, request, which, F, chains):
    """Per frame, the residue and chain values are what the single-structure levels are held to above: the loop over aa.atom_sasa with the
    frame's coordinates and the helper's radii, summed one by one.  (F = 1 below is compared with get_residue_sasa / get_chain_sasa themselves.)"""
    s = request.getfixturevalue(which)
    frames = jittered(s, F)
    assert len(ctx.get_contacts(request.getfixturevalue("ubq"))["model"]) == 532
    got = ctx.residue_sasa_ensemble(s, frames, chains, per_frame=True)
    sel = rc.select_1_to_4(s, chains)
    res, chn = rc.residue_groups(s, sel), rc.chain_groups(s, sel)
    assert got["n_frames"] == F and got["residue_sasa"].shape == (F, len(res)) and got["chain_sasa"].shape == (F, len(chn))
    for f in range(F):
        values = atom_values(ctx, s, sel, "protor", 100, frames[f])
        _, res_sum, _, chn_sum = expected_levels(s, sel, values)
        assert np.array_equal(got["residue_sasa"][f], res_sum), f
        assert np.array_equal(got["chain_sasa"][f], chn_sum), f
    # identity: the rows of the single-structure call
    one = rc.columns(aa.get_residue_sasa(s, chains=chains))
    assert [c.decode() for c in s.strings("chain")[got["res_atoms"]]] == one["chain"] and s.ints("resi")[got["res_atoms"]].tolist() == one["resi"]
    assert got["is_polar"].tolist() == one["is_polar"]
    assert [c.decode() for c in s.strings("chain")[got["chain_atoms"]]] == [c for c, _ in chn]
    # the aggregates, restated from the per-frame values in frame order (as the SAP half of arp_sasa_ensemble_stats)
    w = ec.sap_stats(got["residue_sasa"])
    for k, name in (("mean_sasa", "mean_sap"), ("std_sasa", "std_sap"), ("min_sasa", "min_sap"), ("max_sasa", "max_sap")):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[name]), k
    assert (got["std_sasa"] > 0).sum() > len(res) / 2 and (got["min_sasa"] <= got["mean_sasa"]).all() and (got["mean_sasa"] <= got["max_sasa"]).all()
    for (key, _), mean, rel, ok in zip(res, got["mean_sasa"], got["mean_relative_sasa"], got["relative_valid"]):
        mx = rc.MAX_ASA.get(key[1].upper())
        assert ok == (mx is not None)
        assert np.isnan(rel) if mx is None else rel == mean / np.float32(mx)
    # three passes with a partial last one, one frame per pass, and a repeat: the same bytes
    # (passes are equal but for the last, so 8 frames make 3 + 3 + 2; 4 frames cannot make three passes with a partial last one: they run as
    # 3 + 1 here, and the same input with a fifth frame as 2 + 2 + 1 below)
    want = b"".join(np.ascontiguousarray(got[k]).tobytes() for k in RES_KEYS)
    for per in (3, 1, 0):
        assert per == 0 or (F % per != 0 if per > 1 else F > 1)
        aa.debug_set("ens_chunk_atoms", per * len(sel))
        again = ctx.residue_sasa_ensemble(s, frames, chains, per_frame=True)
        assert b"".join(np.ascontiguousarray(again[k]).tobytes() for k in RES_KEYS) == want, per
    aa.debug_set("ens_chunk_atoms", 0)
    if -(-F // 3) != 3:
        more = jittered(s, F + 1)
        per3 = -(-(F + 1) // 3)
        assert np.array_equal(more[:F], frames) and -(-(F + 1) // per3) == 3 and (F + 1) % per3 != 0
        whole = ctx.residue_sasa_ensemble(s, more, chains, per_frame=True)
        assert np.array_equal(whole["residue_sasa"][:F], got["residue_sasa"]) and np.array_equal(whole["chain_sasa"][:F], got["chain_sasa"])
        assert all(np.array_equal(whole[k], ec.sap_stats(whole["residue_sasa"])[name]) for k, name in (("mean_sasa", "mean_sap"), ("std_sasa", "std_sap")))
        aa.debug_set("ens_chunk_atoms", per3 * len(sel))
        again = ctx.residue_sasa_ensemble(s, more, chains, per_frame=True)
        assert b"".join(np.ascontiguousarray(again[k]).tobytes() for k in RES_KEYS) == b"".join(np.ascontiguousarray(whole[k]).tobytes() for k in RES_KEYS)
        aa.debug_set("ens_chunk_atoms", 0)
    # without the per-frame values nothing else moves
    lean = ctx.residue_sasa_ensemble(s, frames, chains)
    assert "residue_sasa" not in lean and all(np.array_equal(lean[k], got[k], equal_nan=True) for k in RES_KEYS if k != "residue_sasa")
    assert len(ctx.get_contacts(request.getfixturevalue("ubq"))["model"]) == 532
    # the table of the public function
    table, extras = aa.get_residue_sasa_ensemble(s, frames, chains)
    t = rc.columns(table)
    assert list(t) == aa.RESIDUE_ENSEMBLE_SASA_COLUMNS and t["n_frames"] == [F] * len(res)
    assert np.array_equal(np.array(t["mean_sasa"], np.float32), got["mean_sasa"]) and extras["chains"] == [c for c, _ in chn]
    assert np.array_equal(extras["chain_sasa"], got["chain_sasa"])


@pytest.mark.parametrize("which,chains", [("ubq", ""), ("bft", "H,L")])
def test_one_frame_is_the_single_structure_rows(ctx, request, which, chains):
    s = request.getfixturevalue(which)
    got = ctx.residue_sasa_ensemble(s, ec.topology_xyz(s)[None], chains, per_frame=True)
    res = rc.columns(aa.get_relative_sasa(s, chains=chains))
    chn = rc.columns(aa.get_chain_sasa(s, chains=chains))
    want = np.array(res["sasa"], np.float32)
    for k in ("mean_sasa", "min_sasa", "max_sasa"):
        assert np.array_equal(got[k], want), k
    assert np.array_equal(got["residue_sasa"][0], want) and (got["std_sasa"] == 0).all()
    assert np.array_equal(got["chain_sasa"][0], np.array(chn["sasa"], np.float32))
    rel = [None if not ok else float(v) for v, ok in zip(got["mean_relative_sasa"], got["relative_valid"])]
    assert rel == res["relative_sasa"]


def test_sasa_ensemble_with_a_table_name(ctx, ubq):
    frames = jittered(ubq, 3)
    base = ctx.sasa_ensemble(ubq, frames, per_frame=True)
    same = ctx.sasa_ensemble(ubq, frames, per_frame=True, radii="vdw")
    assert ec.result_bytes(base) == ec.result_bytes(same)
    other = ctx.sasa_ensemble(ubq, frames, per_frame=True, radii="protor")
    sel = rc.select_1_to_4(ubq)
    for f in range(3):
        soa_counts = aa.atom_sasa(ctx, *(np.ascontiguousarray(frames[f][sel, k]) for k in range(3)), rc.table_radii(ubq, sel, "protor")[0], None, 1.4, 100)[1]
        assert np.array_equal(other["count"][f], soa_counts)


# ---- 11. the CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_relative_sasa_and_residue_level(tmp_path, ubq_path, ubq):
    import csv

    from arpeggia_amd.__main__ import main

    assert main(["relative-sasa", "-i", ubq_path, "-o", str(tmp_path)]) == 0
    assert main(["sasa", "-i", ubq_path, "-o", str(tmp_path), "-l", "residue", "--radii", "protor", "-f", "res"]) == 0
    assert main(["sasa", "-i", ubq_path, "-o", str(tmp_path), "-l", "chain", "--radii", "protor", "-f", "chain"]) == 0
    with open(tmp_path / "relative_sasa.csv") as f:
        rel = list(csv.DictReader(f))
    with open(tmp_path / "res.csv") as f:
        res = list(csv.DictReader(f))
    with open(tmp_path / "chain.csv") as f:
        chn = list(csv.DictReader(f))
    assert len(rel) == 76 and list(rel[0]) == aa.RELATIVE_SASA_COLUMNS
    assert len(res) == 76 and list(res[0]) == aa.RESIDUE_SASA_COLUMNS
    assert [r["sasa"] for r in rel] == [r["sasa"] for r in res]
    want = rc.columns(aa.get_residue_sasa(ubq))["sasa"]
    assert [np.float32(r["sasa"]) for r in res] == [np.float32(v) for v in want]
    assert len(chn) == 1 and chn[0]["chain"] == "A"
