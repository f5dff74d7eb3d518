"""k_sasa_split (arpeggia_amd/csrc/sasa.inl: the split instantiation of sasa_walk) and what is built on it -- arp_atom_sasa_groups, arp_structure_buried_sasa, arp_dsasa_ensemble -- on
the MI355X.  The yardsticks are never the new kernel: counts come from the numpy restatement of the contract (tests/sasa_restatement.py through
tests/bsa_common.py split_counts), for the decided edge cases from exact rational arithmetic (tests/sasa_edge_cases.py), and on the device from
the existing atom_sasa / atom_sasa_rows / get_residue_sasa / get_dsasa run three times (union, group 1, group 2).  Every comparison is exact:
integer counts equal, f32 areas and totals equal as bit patterns.  tests/test_bsa_host.py holds the preconditions of these inputs."""
import numpy as np
import pytest

import arpeggia_amd as aa
import bsa_common as bc
import ens_sasa_common as ens
import sasa_edge_cases as edge
import sasa_restatement as sr
import synth
from arpeggia_amd import _lib
from conftest import DATA
from ens_sasa_common import bits, three_runs
from ens_sasa_common import bsa_frame_loop as frame_loop

pytestmark = pytest.mark.gpu

NEAR_POINTS = 24


@pytest.fixture(scope="module")
def ctx():
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


def _vdw(elements) -> np.ndarray:
    p = aa.default_params()
    return np.array([p.vdw_radius[_lib.lib.arp_element_class(e)] for e in elements], dtype=np.float32)


_structures = {}


def structure(name: str):
    if name not in _structures:
        _structures[name] = aa.load_model(str(DATA / f"{name}.pdb"))
    return _structures[name]


def structure_inputs(name: str):
    s = structure(name)
    sel, soa = aa.sasa_select(s), s.soa()
    return soa["x"][sel], soa["y"][sel], soa["z"][sel], _vdw(s.strings("element")[sel])


def run(ctx, x, y, z, r, group, probe, n_points=100):
    """One device call with the invariants every result has: the shapes and types, buried = own counts - complex count >= 0, zeros outside the
    groups, areas = the formula on the counts."""
    group = np.asarray(group, np.uint8)
    count, sasa, buried = aa.atom_sasa_groups(ctx, x, y, z, r, group, probe, n_points)
    assert count.shape == sasa.shape == (3, len(group)) and count.dtype == buried.dtype == np.int32 and sasa.dtype == np.float32
    assert np.array_equal(buried, count[1] + count[2] - count[0]) and (buried >= 0).all()
    assert 0 <= count.min() and count.max() <= n_points
    for plane, bit in ((1, 1), (2, 2)):
        assert (count[plane][(group & bit) == 0] == 0).all()
    assert (count[0][group == 0] == 0).all() and (bits(sasa)[:, group == 0] == 0).all()
    R = (np.asarray(r, np.float32) + np.float32(probe)).astype(np.float32)
    assert np.array_equal(bits(sasa)[:, group != 0], bits(bc.areas(R[group != 0], count[:, group != 0], n_points)))
    return count, sasa, buried


def check(ctx, x, y, z, r, group, probe, n_points=100, homes=None):
    """run() against the restatement at `homes` (indices into the inputs; default: every atom with a non-zero mask).  Returns the device counts."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    r, group = np.asarray(r, np.float32), np.asarray(group, np.uint8)
    count, sasa, buried = run(ctx, x, y, z, r, group, probe, n_points)
    homes = np.flatnonzero(group) if homes is None else np.asarray(homes, np.int64)
    R = (r + np.float32(probe)).astype(np.float32)
    want, want_buried = bc.split_counts(x, y, z, R, group, aa.sasa_sphere_points(n_points), homes=homes)
    assert np.array_equal(count[:, homes], want), (count[:, homes] != want).sum(1)
    assert np.array_equal(buried[homes], want_buried)
    return count, sasa, buried


# ---- 1. two atoms ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", bc.PAIR_POINTS)
def test_two_atoms_in_two_groups(ctx, n_points):
    x, y, z, R = bc.pair_on_z(n_points)
    sphere = aa.sasa_sphere_points(n_points)
    assert np.array_equal(sphere, sr.sphere_points(n_points))
    cc = sr.atom_counts(x, y, z, R, sphere)
    assert cc.tolist() == ([0, 1] if n_points == 1 else cc.tolist()) and (n_points == 1 or ((cc > 0) & (cc < n_points)).all())
    for masks in bc.PAIR_MASKS:
        count, sasa, buried = check(ctx, x, y, z, R, masks, 0.0, n_points)
        assert count[0].tolist() == cc.tolist(), masks
        if masks[0] != masks[1]:
            own = count[1] + count[2]
            assert own.tolist() == [n_points, n_points] and buried.tolist() == (n_points - cc).tolist(), masks
        elif masks == (3, 3):  # "/": both groups are the union
            assert count[1].tolist() == count[2].tolist() == cc.tolist() and buried.tolist() == cc.tolist()
        else:
            assert count[1].tolist() == cc.tolist() and count[2].tolist() == [0, 0] and buried.tolist() == [0, 0]
        assert np.array_equal(bits(sasa[0]), bits(sr.sasa_from_counts(R, cc, n_points)))


# ---- 2. the strict edge across groups -----------------------------------------------------------------------------------------------------------------
def test_the_strict_edge_across_groups(ctx):
    """d^2 == R_j^2 is open, one f32 step closer is buried -- in the complex count; the atom's own group never sees the other atom."""
    touching = 0
    for c in edge.on_axis_cases():
        for masks in ((1, 2), (2, 1)):
            count, _, buried = run(ctx, c["x"], c["y"], c["z"], c["radius"], masks, c["probe"], 1)
            home, m = c["home"], c["margin"]
            assert count[0, home] == (0 if m < 0 else 1) and count[0, 1 - home] == 1, c
            assert (count[1] + count[2]).tolist() == [1, 1] and buried.tolist() == (1 - count[0]).tolist(), c
            assert count[1].tolist() == [int(g == 1) for g in masks] and count[2].tolist() == [int(g == 2) for g in masks]
            if c["representable"]:
                assert count[0].tolist() == ([1, 1] if c["step"] >= 0 else ([1, 0] if c["swap"] else [0, 1])), c
                touching += c["touch"]
    assert touching >= 2 * 30


# ---- 3. the f64 band across groups ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def placements():
    sphere = sr.sphere_points(NEAR_POINTS)
    ps = edge.near_sphere_placements(sphere)
    left_out = 0
    for p in ps:
        p["want"], undecided = edge.exact_pair_counts(p["c"], p["R"], sphere)
        left_out += undecided
    assert left_out == 0 and len(ps) == 2100  # every placement is decided by exact arithmetic (tests/test_sasa_edge_host.py): none is left out
    return ps


@pytest.mark.parametrize("same_group", [False, True])
def test_placements_near_the_sphere_across_and_within_groups(ctx, placements, same_group):
    assert np.array_equal(aa.sasa_sphere_points(NEAR_POINTS), sr.sphere_points(NEAR_POINTS))
    checked = 0
    for name, c, R, ps in edge.placement_batches(placements):
        group = np.ones(len(R), np.uint8) if same_group else np.tile(np.array([1, 2], np.uint8), len(ps))
        c = c.astype(np.float64)
        count, _, buried = run(ctx, c[:, 0], c[:, 1], c[:, 2], R, group, 0.0, NEAR_POINTS)
        want = np.array([p["want"] for p in ps], np.int32).reshape(-1)
        assert np.array_equal(count[0], want), name
        if same_group:
            assert np.array_equal(count[1], want) and (count[2] == 0).all() and (buried == 0).all(), name
        else:  # the partner is the only atom near: alone in its group every point is open
            assert np.array_equal(count[1] + count[2], np.full(len(R), NEAR_POINTS)) and np.array_equal(buried, NEAR_POINTS - want), name
        checked += len(ps)
    assert checked == 2 * len(placements)  # once per offset, once in mixed company


# ---- 4. the flush with mixed groups ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.COINCIDENT_N)
def test_flush_on_coincident_atoms_with_mixed_groups(ctx, n):
    x, y, z, r = edge.coincident(n)
    for name, mask in bc.coincident_masks(n).items():
        homes = bc.coincident_homes(mask)
        count, _, buried = check(ctx, x, y, z, r, mask, 0.0, homes=homes)
        grid = mask != 0
        assert (count[0][grid] == count[0][grid][0]).all() and 0 < count[0][grid][0] < 100, name
        if name.startswith("lone"):  # every list entry buries the lone atom in the complex, none in its own group: its lane must stay open through every flush
            g = 1 if name == "lone1" else 2
            lone = int(np.flatnonzero(mask == g)[0])
            assert count[g, lone] == 100 and buried[lone] == 100 - count[0, lone] and (np.delete(buried, lone) == 0).all(), name


@pytest.mark.parametrize("probe", [5.0, 8.0])
def test_flush_on_1ubq_with_random_masks(ctx, probe):
    x, y, z, r = structure_inputs("1ubq")
    mask = bc.random_masks(len(x), int(probe), with_zero=False)
    count, sasa, _ = check(ctx, x, y, z, r, mask, probe)
    nb, homes = bc.crowded_homes(x, y, z, (r + np.float32(probe)).astype(np.float32), mask, per_group=len(x))
    crowded = np.concatenate([homes[1], homes[2]])
    assert (count[:, crowded] > 0).any(1).all()
    want_count, want_sasa = three_runs(ctx, x, y, z, r, mask, probe)
    assert np.array_equal(count, want_count) and np.array_equal(bits(sasa), bits(want_sasa))
    assert aa.sasa_tests(ctx) > 0


def test_masked_out_atoms_neither_bury_nor_are_buried(ctx):
    x, y, z, r = structure_inputs("1ubq")
    mask = bc.random_masks(len(x), 77)
    assert (mask == 0).sum() > 100
    r = r.copy()
    r[mask == 0] = np.float32(50.0)  # the radius of an atom outside the groups must not matter, not even as the largest
    count, sasa, _ = check(ctx, x, y, z, r, mask, 1.4)
    want_count, want_sasa = three_runs(ctx, x, y, z, r, mask, 1.4)
    assert np.array_equal(count, want_count) and np.array_equal(bits(sasa), bits(want_sasa))


# ---- 5. the three-run identity on files -------------------------------------------------------------------------------------------------------------------
def _chains(s, groups):
    g1, g2 = aa.parse_groups(sorted(set(c.decode() for c in s.strings("chain"))), groups)
    return ",".join(sorted(g1)), ",".join(sorted(g2)), ",".join(sorted(set(g1) | set(g2)))


def _table_columns(t):
    t = t if hasattr(t, "column") and not hasattr(t, "to_arrow") else t.to_arrow()
    return {k: t.column(k).to_pylist() for k in t.column_names}


def check_file(ctx, s, groups, model_num=0, radii=None, probe=1.4, n_points=100):
    c1, c2, cu = _chains(s, groups)
    got = ctx.buried_sasa(s, groups, probe, n_points, model_num, radii)
    rows = {c: aa.api.atom_sasa_rows(s, probe, n_points, model_num, True, c, radii=radii) for c in {c1, c2, cu}}
    idx, sasa_u, count_u = rows[cu]
    assert np.array_equal(got["atoms"], idx) and len(idx) > 20
    assert np.array_equal(got["count"][0], count_u) and np.array_equal(bits(got["sasa"][0]), bits(sasa_u))
    for plane, c in ((1, c1), (2, c2)):
        member = np.isin(idx, rows[c][0])
        assert np.array_equal(idx[member], rows[c][0]) and np.array_equal((got["group"] & plane) != 0, member)
        assert np.array_equal(got["count"][plane][member], rows[c][2]) and np.array_equal(bits(got["sasa"][plane][member]), bits(rows[c][1]))
        assert (got["count"][plane][~member] == 0).all() and (bits(got["sasa"][plane][~member]) == 0).all()
    assert np.array_equal(got["buried"], got["count"][1] + got["count"][2] - got["count"][0]) and (got["buried"] >= 0).all()
    # the scalar: get_dsasa, bit for bit
    want = np.float32(aa.get_dsasa(s, groups, probe, n_points, model_num, radii=radii))
    assert np.float32(got["dsasa"]).view(np.uint32) == want.view(np.uint32) == got["totals"][3:].view(np.uint32)[0], (got["dsasa"], want)
    return got, (c1, c2, cu)


@pytest.mark.parametrize("groups", bc.FILE_GROUPS)
def test_three_run_identity_on_6bft(ctx, groups):
    s = structure("6bft")
    for radii in (None, "protor"):
        got, (c1, c2, cu) = check_file(ctx, s, groups, radii=radii)
        # the residue rows: get_residue_sasa's on the same chains, row for row (it needs a named table)
        table = radii or "vdw"
        res = got if radii else ctx.buried_sasa(s, groups, radii="vdw")
        if not radii:
            assert np.array_equal(bits(res["sasa"]), bits(got["sasa"])) and res["dsasa"] == got["dsasa"]  # "vdw" names the default table
        want_u = aa.api.level_sasa_rows(s, "residue", chains=cu, radii=table)
        assert np.array_equal(res["res_atoms"], want_u["atoms"]) and np.array_equal(bits(res["res_sasa"][0]), bits(want_u["sasa"]))
        group_of = dict(zip(res["atoms"].tolist(), res["group"].tolist()))
        res_group = np.array([group_of[a] for a in res["res_atoms"].tolist()], np.uint8)
        for plane, c in ((1, c1), (2, c2)):
            want_g = aa.api.level_sasa_rows(s, "residue", chains=c, radii=table)
            member = (res_group & plane) != 0
            assert np.array_equal(res["res_atoms"][member], want_g["atoms"]) and np.array_equal(bits(res["res_sasa"][plane][member]), bits(want_g["sasa"]))
            assert (bits(res["res_sasa"][plane][~member]) == 0).all()
        nb = np.zeros(len(res["res_atoms"]), np.int64)
        res_of_atom = {}
        resid = list(zip(s.strings("chain").tolist(), s.ints("resi").tolist(), s.strings("insertion").tolist()))
        for k, a in enumerate(res["res_atoms"].tolist()):
            res_of_atom[resid[a]] = k
        for a, b in zip(res["atoms"].tolist(), res["buried"].tolist()):
            nb[res_of_atom[resid[a]]] += b > 0
        assert np.array_equal(res["res_buried_atoms"], nb)
    if groups == "C/H,L":
        assert abs(got["dsasa"] - 1650.0) <= 50.0  # (ProtOr radii here; van der Waals below) the reference's own pin for this file
        assert abs(ctx.buried_sasa(s, groups)["dsasa"] - 1650.0) <= 50.0
    if groups == "/":
        assert (got["group"] == 3).all() and np.array_equal(got["buried"], got["count"][0])


def test_tables_on_6bft(ctx):
    s = structure("6bft")
    raw = ctx.buried_sasa(s, "C/H,L")
    table, total = aa.get_buried_sasa(s, "C/H,L")
    assert total == raw["dsasa"] == aa.get_dsasa(s, "C/H,L")
    cols = _table_columns(table)
    assert list(cols) == aa.BURIED_ATOM_COLUMNS and len(table) == len(raw["atoms"])
    ref = _table_columns(aa.get_atom_sasa(s, chains="C,H,L"))
    for k in ("atomi", "chain", "resn", "resi", "insertion", "altloc", "atomn"):
        assert cols[k] == ref[k], k
    assert cols["sasa_complex"] == ref["sasa"] and cols["group"] == raw["group"].tolist()
    in1 = (raw["group"] & 1) != 0
    assert [v is None for v in cols["sasa_group1"]] == (~in1).tolist() and [v is None for v in cols["sasa_group2"]] == in1.tolist()
    own = np.where(in1, raw["sasa"][1], raw["sasa"][2]).astype(np.float32)
    assert np.array_equal(bits(np.array(cols["buried"], np.float32)), bits(own - raw["sasa"][0]))
    assert (np.array(cols["buried"]) > 0).sum() > 100 and ((np.array(cols["buried"]) > 0) == (raw["buried"] > 0)).all()
    rtable, rtotal = aa.get_buried_sasa(s, "C/H,L", level="residue", radii="protor")
    rcols = _table_columns(rtable)
    ref = _table_columns(aa.get_residue_sasa(s, chains="C,H,L", radii="protor"))
    assert list(rcols) == aa.BURIED_RESIDUE_COLUMNS and rtotal == aa.get_dsasa(s, "C/H,L", radii="protor")
    for k in ("chain", "resn", "resi", "insertion"):
        assert rcols[k] == ref[k], k
    assert rcols["sasa_complex"] == ref["sasa"] and sum(rcols["n_buried_atoms"]) == int((ctx.buried_sasa(s, "C/H,L", radii="protor")["buried"] > 0).sum())
    assert 20 < sum(v > 0 for v in rcols["n_buried_atoms"]) < 120  # an epitope and a paratope, not the whole complex


@pytest.mark.parametrize("model_num", [1, 2])
def test_three_run_identity_on_the_models_of_hand7(ctx, model_num):
    s = structure("hand7")
    got, _ = check_file(ctx, s, "/", model_num=model_num)
    other, _ = check_file(ctx, s, "/", model_num=3 - model_num)
    assert len(got["atoms"]) == len(other["atoms"]) and not np.array_equal(got["atoms"], other["atoms"])
    check_file(ctx, s, "/", model_num=model_num, radii="protor", probe=2.0, n_points=257)


# ---- 6. packed frames ------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,groups,probe", [("6bft", "C/H,L", 1.4), ("6bft", "C/H,L", 6.0), ("6bft", "A,B/A,G", 1.4), ("hand7", "/", 1.4), ("1ubq", "/", 6.0)])
def test_packed_frames_equal_the_frame_loop(ctx, name, groups, probe):
    s = structure(name)
    frames = ens.jittered(s, 3, seed=41)
    n_points = 100
    try:
        got = ctx.dsasa_ensemble(s, frames, groups, probe, n_points, per_frame=True)
        m = len(got["atoms"])
        for budget in (m, 2 * m):  # one and two frames per pass: byte-identical
            aa.debug_set("ens_chunk_atoms", budget)
            assert ens.result_bytes(ctx.dsasa_ensemble(s, frames, groups, probe, n_points, per_frame=True)) == ens.result_bytes(got), budget
    finally:
        aa.debug_set("ens_chunk_atoms", 0)
    assert got["n_frames"] == 3 and got["buried"].shape == (3, m) and m > 20
    loop = frame_loop(ctx, s, got, frames, probe, n_points)
    assert np.array_equal(got["buried"], loop["buried"])
    for k in ("total_complex", "total_g1", "total_g2", "dsasa"):
        assert np.array_equal(bits(got[k]), bits(loop[k])), k
    b = loop["buried"].astype(np.int64)
    assert np.array_equal(got["sum_buried"], b.sum(0).astype(np.uint64)) and np.array_equal(got["sum_buried_sq"], (b * b).sum(0).astype(np.uint64))
    assert np.array_equal(got["min_buried"], b.min(0)) and np.array_equal(got["max_buried"], b.max(0))
    assert np.array_equal(got["frames_buried"], (b > 0).sum(0).astype(np.uint32))
    assert (b > 0).any() and (b.min(0) != b.max(0)).any()
    if probe == 6.0:
        x, y, z = (np.ascontiguousarray(frames[0][got["atoms"].astype(np.int64), k]) for k in range(3))
        assert (edge.neighbour_counts(x, y, z, got["R"]) > 256).sum() > 100  # the flush happens under per_model
    # the tables on top: the statistics from the integers, on the host
    ft, at = aa.get_dsasa_ensemble(s, frames, groups, probe, n_points)
    fcols, acols = _table_columns(ft), _table_columns(at)
    assert list(fcols) == aa.DSASA_FRAME_COLUMNS and list(acols) == aa.DSASA_ENSEMBLE_COLUMNS and fcols["frame"] == [0, 1, 2]
    assert np.array_equal(bits(np.array(fcols["dsasa"], np.float32)), bits(loop["dsasa"]))
    want = bc.buried_stats(3, got["R"], n_points, loop["buried"])
    for k in ("buried_mean", "buried_std", "buried_min", "buried_max"):
        assert np.array_equal(bits(np.array(acols[k], np.float32)), bits(want[k])), k
    assert acols["occupancy"] == want["occupancy"].tolist() and acols["group"] == got["group"].tolist()


def test_one_frame_is_the_single_structure_call(ctx):
    s = structure("6bft")
    got = ctx.dsasa_ensemble(s, None, "C/H,L", per_frame=True)  # frames None: the models of the file
    one = ctx.buried_sasa(s, "C/H,L")
    order = np.argsort(one["atoms"], kind="stable")
    assert got["n_frames"] == 1 and np.array_equal(got["atoms"], one["atoms"][order])
    assert np.array_equal(got["buried"][0], one["buried"][order])
    assert got["dsasa"][0] == np.float32(aa.get_dsasa(s, "C/H,L"))


def test_1ubq_split_by_residue_halves_over_jittered_frames(ctx):
    """The artificial split at array level: a one-chain structure, masks by residue number, every frame against the three runs."""
    s = structure("1ubq")
    sel = aa.sasa_select(s)
    mask = bc.halves_by_residue(s.ints("resi")[sel])
    r = _vdw(s.strings("element")[sel])
    frames = ens.jittered(s, 3, seed=41)
    for f, probe in ((0, 1.4), (1, 1.4), (2, 6.0)):
        x, y, z = (np.ascontiguousarray(frames[f][sel, k]) for k in range(3))
        count, sasa, buried = check(ctx, x, y, z, r, mask, probe)
        want_count, want_sasa = three_runs(ctx, x, y, z, r, mask, probe)
        assert np.array_equal(count, want_count) and np.array_equal(bits(sasa), bits(want_sasa))
        assert (buried > 0).sum() > 50


# ---- 7. the cell order changes nothing -------------------------------------------------------------------------------------------------------------------
def test_forced_y_strips_change_nothing(ctx):
    rec = synth.gen_s1(40_000)
    r = _vdw(rec["element"])
    mask = bc.random_masks(len(r), 11)
    s = structure("6bft")
    frames = ens.jittered(s, 2, seed=5)
    base = aa.atom_sasa_groups(ctx, rec["x"], rec["y"], rec["z"], r, mask)
    base_file, base_ens = ctx.buried_sasa(s, "C/H,L"), ctx.dsasa_ensemble(s, frames, "C/H,L", per_frame=True)
    aa.debug_set("strip_rows", 4)
    try:
        strips = aa.atom_sasa_groups(ctx, rec["x"], rec["y"], rec["z"], r, mask)
        strips_file, strips_ens = ctx.buried_sasa(s, "C/H,L"), ctx.dsasa_ensemble(s, frames, "C/H,L", per_frame=True)
    finally:
        aa.debug_set("strip_rows", 0)
    again = aa.atom_sasa_groups(ctx, rec["x"], rec["y"], rec["z"], r, mask)
    for a, b, c in zip(base, strips, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert ens.result_bytes(base_file) == ens.result_bytes(strips_file) and ens.result_bytes(base_ens) == ens.result_bytes(strips_ens)
    assert (base[2] > 0).sum() > 1000


# ---- 8. more than a PDB file: the multi-block grid ----------------------------------------------------------------------------------------------------------
def test_forty_thousand_atoms_split_by_copy_parity(ctx):
    rec = synth.gen_s1(40_000)
    r = _vdw(rec["element"])
    n_template = len(synth.read_pdb_records(DATA / "1ubq.pdb")["x"])
    mask = (1 + (np.arange(len(r)) // n_template) % 2).astype(np.uint8)  # neighbouring copies of the template alternate between the groups
    assert (mask == 1).sum() > 15_000 and (mask == 2).sum() > 15_000
    R = (r + np.float32(1.4)).astype(np.float32)
    nb = edge.neighbour_counts(rec["x"], rec["y"], rec["z"], R)
    homes = edge.homes_sample(nb, 32, 480, seed=8)
    assert nb.max() in nb[homes]
    count, _, buried = check(ctx, rec["x"], rec["y"], rec["z"], r, mask, 1.4, homes=homes)
    assert (buried[homes] > 0).any() and (buried[homes] == 0).any() and (buried > 0).sum() > 500
    assert aa.sasa_tests(ctx) > 100 * len(r)
