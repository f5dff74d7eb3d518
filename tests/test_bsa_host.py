"""Buried surface per atom and residue, dSASA across frames (arp_atom_sasa_groups, arp_structure_buried_sasa, arp_dsasa_ensemble): everything
that is decided before the device is touched -- the argument checks of the three entry points through a NULL context, the CLI, the exports --
the host-side statistics against their restatement, and the preconditions of the device inputs of tests/test_bsa_gpu.py: a device test must
not be able to pass without reaching the path it is there for.  No compute call is made."""
from __future__ import annotations

import re

import numpy as np
import pytest

import arpeggia_amd as aa
import bsa_common as bc
import ens_sasa_common as ens
import sasa_edge_cases as edge
import sasa_restatement as sr
from arpeggia_amd import _lib
from arpeggia_amd.api import _buried_sasa, _dsasa_ensemble
from conftest import DATA, ROOT


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


@pytest.fixture(scope="module")
def bft(bft_path):
    return aa.load_model(bft_path)


def refused(fn, *args, status=_lib.ARP_ERR_BAD_INPUT, match: str | None = None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)
    return str(e.value)


def _vdw(elements) -> np.ndarray:
    p = aa.default_params()
    return np.array([p.vdw_radius[_lib.lib.arp_element_class(e)] for e in elements], dtype=np.float32)


def structure_inputs(name: str):
    s = aa.load_model(str(DATA / f"{name}.pdb"))
    sel, soa = aa.sasa_select(s), s.soa()
    return s, sel, soa["x"][sel], soa["y"][sel], soa["z"][sel], _vdw(s.strings("element")[sel])


# ---- the surface ------------------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = {"arp_atom_sasa_groups", "arp_structure_buried_sasa", "arp_dsasa_ensemble", "arp_dsasa_total"}


def test_header_lib_and_package_agree():
    header = (ROOT / "include" / "arpeggia_amd.h").read_text()
    declared = set(re.findall(r"\b(arp_[a-z_0-9]+)\s*\(", header))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_lib.EXPORTS) and sorted(_lib.EXPORTS) == sorted(declared)
    assert _lib.lib.arp_api_version() == 2  # additive: the version stays
    for name in ("atom_sasa_groups", "get_buried_sasa", "buried_sasa", "get_dsasa_ensemble", "dsasa_ensemble", "dsasa_ensemble_stats", "dsasa_total"):
        assert callable(getattr(aa, name)), name
    assert callable(aa.Context.buried_sasa) and callable(aa.Context.dsasa_ensemble)
    assert aa.BURIED_ATOM_COLUMNS == ["atomi", "chain", "resn", "resi", "insertion", "altloc", "atomn", "group", "sasa_complex", "sasa_group1", "sasa_group2", "buried"]
    assert aa.BURIED_RESIDUE_COLUMNS == ["chain", "resn", "resi", "insertion", "group", "sasa_complex", "sasa_group1", "sasa_group2", "buried", "n_buried_atoms"]
    assert aa.DSASA_FRAME_COLUMNS == ["frame", "total_complex", "total_group1", "total_group2", "dsasa"]
    assert aa.DSASA_ENSEMBLE_COLUMNS[:7] == aa.ENSEMBLE_SASA_COLUMNS[:7]
    assert aa.DSASA_ENSEMBLE_COLUMNS[7:] == ["group", "n_frames", "buried_mean", "buried_std", "buried_min", "buried_max", "occupancy"]


def test_cli_dsasa_level_and_dsasa_ensemble(tmp_path, ubq_path):
    from arpeggia_amd.__main__ import build_parser, main

    a = build_parser().parse_args(["dsasa", "-i", "x.pdb", "-g", "A/B"])
    assert (a.level, a.output, a.filename, a.output_format, a.probe_radius, a.n_points, a.model_num, a.radii) == ("total", None, "dsasa", "csv", 1.4, 100, 0, None)
    a = build_parser().parse_args(["dsasa", "-i", "x.pdb", "-g", "A/B", "-l", "RESIDUE", "-o", "d", "-f", "f", "-t", "PARQUET", "--radii", "protor"])
    assert (a.level, str(a.output), a.filename, a.output_format, a.radii) == ("residue", "d", "f", "parquet", "protor")
    assert build_parser().parse_args(["dsasa", "-i", "x.pdb", "-g", "A/B", "--level", "atom"]).level == "atom"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["dsasa", "-i", "x.pdb", "-g", "A/B", "-l", "chain"])
    a = build_parser().parse_args(["dsasa-ensemble", "-i", "x.pdb", "-o", str(tmp_path), "-g", "H,L/C"])
    assert (a.groups, a.filename, a.output_format, a.probe_radius, a.n_points, a.num_threads, a.radii) == ("H,L/C", "dsasa_ensemble", "csv", 1.4, 100, 1, None)
    assert not hasattr(a, "model_num")
    a = build_parser().parse_args(["dsasa-ensemble", "-i", "x.pdb", "-o", "d", "-g", "/", "-f", "f", "-t", "NDJSON", "-r", "1.2", "-n", "64", "-j", "4", "--radii", "vdw"])
    assert (a.filename, a.output_format, a.probe_radius, a.n_points, a.num_threads, a.radii) == ("f", "ndjson", 1.2, 64, 4, "vdw")
    for argv in (["dsasa-ensemble", "-i", "x.pdb", "-o", "d"], ["dsasa-ensemble", "-i", "x.pdb", "-o", "d", "-g", "/", "-m", "1"]):
        with pytest.raises(SystemExit):  # -g is required; no --model: the models are the frames
            build_parser().parse_args(argv)
    assert main(["dsasa-ensemble", "-i", str(tmp_path / "none.pdb"), "-o", str(tmp_path), "-g", "/"]) == 1
    assert main(["dsasa", "-i", str(tmp_path / "none.pdb"), "-g", "/", "-l", "atom"]) == 1
    assert main(["dsasa", "-i", ubq_path, "-g", "/", "-l", "atom"]) == 2  # a table needs --output


# ---- argument checks without a device ------------------------------------------------------------------------------------------------------------
def groups_call(group, radius=None, probe=1.4, n_points=100):
    n = len(group)
    return aa.atom_sasa_groups(None, np.arange(n) * 3.0, np.zeros(n), np.zeros(n), np.full(n, 1.7, np.float32) if radius is None else radius, group,
                               probe, n_points)


def test_atom_sasa_groups_argument_checks():
    refused(groups_call, [1, 2, 4], match="atom 2: group mask 4")
    refused(groups_call, [255], match="group mask 255")
    for n_points in (0, -5, 4097):
        refused(groups_call, [1, 2], n_points=n_points, match="n_points must be 1..4096")
    for probe in (-0.1, np.nan, np.inf):
        refused(groups_call, [1, 2], probe=probe, match="probe radius")
    for bad in (-1.0, np.nan, np.inf):
        refused(groups_call, [1, 2], radius=np.array([1.0, bad], np.float32), match="atom 1: radius")
        refused(groups_call, [1, 0], radius=np.array([1.0, bad], np.float32), match="null context")  # out of the grid: its radius is not read
    refused(groups_call, [1, 2, 3, 0], match="null context")  # every check passed: the missing context is what is left
    x = np.zeros(2)
    f, g = np.ones(2, np.float32), np.ones(2, np.uint8)
    dp, fp, ip, bp = (_lib.C.POINTER(t) for t in (_lib.C.c_double, _lib.C.c_float, _lib.C.c_int32, _lib.C.c_uint8))
    ok = [x.ctypes.data_as(dp)] * 3 + [f.ctypes.data_as(fp), g.ctypes.data_as(bp), _lib.C.c_float(1.4), 100, np.zeros(6, "<i4").ctypes.data_as(ip),
                                      np.zeros(6, "<f4").ctypes.data_as(fp), np.zeros(2, "<i4").ctypes.data_as(ip)]
    for k in (0, 1, 2, 3, 4, 7, 8, 9):  # every pointer in turn
        args = list(ok)
        args[k] = None
        assert _lib.lib.arp_atom_sasa_groups(None, 2, *args) == _lib.ARP_ERR_BAD_INPUT and b"null argument" in _lib.lib.arp_last_error()
    assert _lib.lib.arp_atom_sasa_groups(None, 0, *([None] * 5), _lib.C.c_float(1.4), 100, None, None, None) == _lib.ARP_ERR_BAD_INPUT  # n = 0: only the context is missing
    assert b"null context" in _lib.lib.arp_last_error()


def buried_check(s, groups="/", probe=1.4, n_points=100, model_num=0, radii=None):
    return _buried_sasa(None, s, groups, probe, n_points, model_num, radii)


def ensemble_check(s, frames=None, groups="/", probe=1.4, n_points=100, radii=None):
    return _dsasa_ensemble(None, s, frames, groups, probe, n_points, radii, False)


def test_structure_entry_points_argument_checks(bft, ubq):
    frames = ens.topology_xyz(ubq)[None].repeat(2, 0)
    for check, s, extra in ((buried_check, bft, {}), (ensemble_check, ubq, {"frames": frames})):
        refused(check, s, groups="A,B", status=_lib.ARP_ERR_BAD_GROUPS, match="Invalid chain groups format! Use '/' for all-to-all comparisons.", **extra)
        every = ",".join(sorted(set(c.decode() for c in s.strings("chain"))))
        refused(check, s, groups=every + "/", status=_lib.ARP_ERR_EMPTY_GROUPS, match="Empty chain groups!", **extra)  # the rest of every chain is no chain
        for n_points in (0, 4097):
            refused(check, s, n_points=n_points, match="n_points must be 1..4096", **extra)
        for probe in (-0.1, np.nan):
            refused(check, s, probe=probe, match="probe radius", **extra)
        with pytest.raises(ValueError, match="Invalid radii"):
            check(s, radii="chothia", **extra)
    refused(buried_check, bft, "C/H,L", match="null argument")  # every check passed: the missing context is what is left
    refused(aa.get_buried_sasa, bft, "A,B", status=_lib.ARP_ERR_BAD_GROUPS)  # an input error comes ahead of a missing device
    refused(aa.get_dsasa_ensemble, ubq, frames, "/A", status=_lib.ARP_ERR_EMPTY_GROUPS)
    with pytest.raises(ValueError, match="Invalid level"):
        aa.get_buried_sasa(bft, "C/H,L", level="chain")
    # null outputs
    n, q = _lib.C.c_uint64(), _lib.C.c_uint64()
    assert _lib.lib.arp_structure_buried_sasa(None, bft._h, b"C/H,L", _lib.C.c_float(1.4), 100, 0, 0, _lib.C.byref(n), *([None] * 5), _lib.C.byref(q), *([None] * 4)) == _lib.ARP_ERR_BAD_INPUT
    assert b"null argument" in _lib.lib.arp_last_error()
    assert _lib.lib.arp_dsasa_ensemble(None, ubq._h, 0, None, b"/", _lib.C.c_float(1.4), 100, 0, None, None, *([None] * 13)) == _lib.ARP_ERR_BAD_INPUT
    assert b"null argument" in _lib.lib.arp_last_error()


def test_ensemble_checks_and_selection(bft, ubq):
    r = ensemble_check(bft, groups="C/H,L")
    chains = bft.strings("chain")[r["atoms"]]
    assert r["n_frames"] == 1 and set(chains.tolist()) == {b"C", b"H", b"L"}
    assert np.array_equal(r["group"], np.where(chains == b"C", 1, 2)) and (np.diff(r["atoms"].astype(np.int64)) > 0).all()
    assert np.array_equal(r["R"], (_vdw(bft.strings("element")[r["atoms"]]) + np.float32(1.4)).astype(np.float32))
    assert (ensemble_check(bft, groups="/")["group"] == 3).all()
    part = ensemble_check(bft, groups="A,B/A,G")
    ch = bft.strings("chain")[part["atoms"]]
    assert np.array_equal(part["group"], np.select([ch == b"A", ch == b"B", ch == b"G"], [3, 1, 2]))
    rest = ensemble_check(bft, groups="C/")
    assert set(bft.strings("chain")[rest["atoms"]][rest["group"] == 2].tolist()) == {b"A", b"B", b"G", b"H", b"L"}
    sel = aa.sasa_select(ubq)
    assert np.array_equal(ensemble_check(ubq, ens.topology_xyz(ubq)[None].repeat(3, 0))["atoms"], sel)
    refused(ensemble_check, ubq, np.zeros((0, 660, 3)), match="at least one frame")
    refused(ensemble_check, ubq, np.zeros((2, 5, 3)), match="shape")
    f = ens.topology_xyz(ubq)[None].repeat(3, 0)
    f[2, 17, 1] = np.nan
    refused(ensemble_check, ubq, f, match="frame 2, atom 17")


def test_a_negative_total_is_the_reference_error():
    assert aa.dsasa_total(100.0, 60.0, 70.0) == 30.0
    assert aa.dsasa_total(130.0, 60.0, 70.0) == 0.0
    refused(aa.dsasa_total, 130.5, 60.0, 70.0, match="Negative dSASA calculated. Please check the input file and chain groups.")
    # f32, in the order g1 + g2 - complex: 2^24 + 1 is lost before the subtraction
    assert aa.dsasa_total(16777216.0, 16777216.0, 1.0) == 0.0


# ---- the host-side statistics ------------------------------------------------------------------------------------------------------------------------
def test_statistics_from_hand_made_accumulators():
    buried = np.array([[0, 3, 100, 7, 0], [0, 0, 100, 9, 1], [0, 5, 100, 2, 0], [0, 0, 100, 4096, 0]], np.int64)
    F, m = buried.shape
    R = np.array([3.1, 3.25, 2.82, 1.4, 0.0], np.float32)
    got = aa.dsasa_ensemble_stats(F, R, 100, buried.sum(0), (buried * buried).sum(0), buried.min(0), buried.max(0), (buried > 0).sum(0))
    want = bc.buried_stats(F, R, 100, buried)
    for k in ("buried_mean", "buried_std", "buried_min", "buried_max"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert got["occupancy"].tolist() == want["occupancy"].tolist() == [0.0, 0.5, 1.0, 1.0, 0.25]
    assert got["buried_std"][2] == 0.0 and got["buried_mean"][0] == 0.0 and (got["buried_mean"][4], got["buried_max"][4]) == (0.0, 0.0)
    point = (bc.FOUR_PI * float(R[1])) * float(R[1]) / 100.0
    assert got["buried_mean"][1] == np.float32(point * 2.0) and got["buried_max"][1] == np.float32(point * 5.0)
    # sums far above 2^32: the integer accumulators are 64-bit
    big = aa.dsasa_ensemble_stats(10 ** 6, R[:1], 4096, [4096 * 10 ** 6], [4096 * 4096 * 10 ** 6], [4096], [4096], [10 ** 6])
    assert big["buried_std"][0] == 0.0 and big["buried_mean"][0] == big["buried_max"][0] and big["occupancy"][0] == 1.0


# ---- preconditions of the device cases -------------------------------------------------------------------------------------------------------------
def test_the_pair_on_z_is_partly_buried_at_every_point_count():
    """GPU case 1.  One point: the pole of the lower atom is the contact point and is buried, the upper atom's pole is open.  From 63 points
    on some but not all points of each atom are buried."""
    for n_points in bc.PAIR_POINTS:
        x, y, z, R = bc.pair_on_z(n_points)
        sphere = sr.sphere_points(n_points)
        assert sphere[0].tolist() == [0.0, 0.0, 1.0]
        c = sr.atom_counts(x, y, z, R, sphere)
        if n_points == 1:
            assert c.tolist() == [0, 1]
        else:
            assert (c > 0).all() and (c < n_points).all(), c
        assert c.tolist() == edge.exact_pair_counts(np.stack([edge.f32(x), edge.f32(y), edge.f32(z)], 1), R, sphere)[0]
        for masks in bc.PAIR_MASKS:
            counts, buried = bc.split_counts(x, y, z, R, masks, sphere)
            assert counts[0].tolist() == c.tolist()
            if masks[0] != masks[1]:  # alone in its group: nothing buries it there
                assert buried.tolist() == (n_points - c).tolist() and counts[1].tolist() == [n_points * (masks[0] == 1), n_points * (masks[1] == 1)]
            elif masks == (3, 3):
                assert buried.tolist() == c.tolist() and counts[1].tolist() == counts[2].tolist() == c.tolist()
            else:
                assert buried.tolist() == [0, 0] and counts[2].tolist() == [0, 0]


@pytest.mark.parametrize("n", bc.COINCIDENT_N)
def test_coincident_mask_sets_flush_in_both_groups(n):
    """GPU case 4.  Every atom has n - 1 > 256 neighbours whatever its mask says; the lone atom of a group keeps every point in its own count
    although every list entry buries it in the complex."""
    x, y, z, r = edge.coincident(n)
    sphere = sr.sphere_points(100)
    sets = bc.coincident_masks(n)
    assert list(sets) == ["alternating", "lone1", "lone2", "random1", "random2", "random3"]
    pair = int(sr.atom_counts(x[:2], y[:2], z[:2], r[:2], sphere)[0])
    assert 0 < pair < 100
    for name, mask in sets.items():
        grid = np.flatnonzero(mask)
        assert (edge.neighbour_counts(x[grid], y[grid], z[grid], r[grid]) == len(grid) - 1).all()
        if name.startswith("random"):
            assert set(mask.tolist()) == {0, 1, 2, 3}
            # a quarter of the atoms is out: 300 atoms leave a list that is nearly full and is not flushed, 600 and 1100 flush
            assert (len(grid) - 1 > 256) == (n > 300) and len(grid) > 200
        else:
            assert len(grid) - 1 > 256
        homes = bc.coincident_homes(mask)
        assert set(mask[homes].tolist()) == set(mask[grid].tolist())
        counts, buried = bc.split_counts(x, y, z, r, mask, sphere, homes=homes)
        assert (counts[0] == pair).all()
        if name.startswith("lone"):
            g = 1 if name == "lone1" else 2
            lone = int(np.flatnonzero(mask == g)[0])
            at = int(np.flatnonzero(homes == lone)[0])
            assert counts[g, at] == 100 and buried[at] == 100 - pair and (np.delete(buried, at) == 0).all()
        else:
            assert (buried == np.where(mask[homes] == 3, pair, 0)).all()  # in both groups: both own counts are the pair's


@pytest.mark.parametrize("probe", [5.0, 8.0])
def test_1ubq_with_random_masks_flushes_with_open_points_in_every_count(probe):
    """GPU case 4: homes with more than 256 neighbours exist in both groups, and some of them keep open points in each of the three counts."""
    _, _, x, y, z, r = structure_inputs("1ubq")
    R = (r + np.float32(probe)).astype(np.float32)
    mask = bc.random_masks(len(x), int(probe), with_zero=False)
    assert set(mask.tolist()) == {1, 2, 3}
    nb, homes = bc.crowded_homes(x, y, z, R, mask, per_group=len(x))
    sphere = sr.sphere_points(100)
    open_in = np.zeros(3, np.int64)
    for g in (1, 2):
        assert len(homes[g]) >= 100 and (nb[homes[g]] > 256).all() and ((mask[homes[g]] & g) != 0).all()
        counts, buried = bc.split_counts(x, y, z, R, mask, sphere, homes=homes[g])
        open_in += (counts > 0).any(1)
        assert (counts[g] > 0).any() and (buried > 0).any()  # an own count that outlives the flush, with points the other group buries
        assert (counts[g] >= counts[0]).all() and (buried >= 0).all()
    assert (open_in > 0).all(), open_in  # complex, group 1, group 2: each keeps open points at some crowded home


def test_file_groups_parse_to_the_sets_the_device_test_compares(bft):
    """GPU case 5."""
    chains = sorted(set(c.decode() for c in bft.strings("chain")))
    assert chains == ["A", "B", "C", "G", "H", "L"]
    want = {"C/H,L": (["C"], ["H", "L"]), "H/L": (["H"], ["L"]), "A,B/G": (["A", "B"], ["G"]), "/": (chains, chains), "A,B/A,G": (["A", "B"], ["A", "G"]),
            "C/": (["C"], ["A", "B", "G", "H", "L"])}
    assert set(want) == set(bc.FILE_GROUPS)
    for groups, (g1, g2) in want.items():
        got = aa.parse_groups(chains, groups)
        assert (sorted(got[0]), sorted(got[1])) == (g1, g2), groups
    hand = aa.load_model(str(DATA / "hand7.pdb"))
    assert len(set(hand.ints("model").tolist())) == 2 and len(aa.sasa_select(hand, model_num=1)) == len(aa.sasa_select(hand, model_num=2)) > 20


def test_packed_frame_inputs(bft, ubq):
    """GPU case 6: the frames differ, the artificial split of 1ubq has two sizeable halves in contact, and probe 6.0 fills the list."""
    frames = ens.jittered(ubq, 3, seed=41)
    assert frames.shape == (3, 660, 3) and not np.array_equal(frames[0], frames[1])
    sel = aa.sasa_select(ubq)
    mask = bc.halves_by_residue(ubq.ints("resi")[sel])
    assert min((mask == 1).sum(), (mask == 2).sum()) > 250 and set(mask.tolist()) == {1, 2}
    x, y, z = (np.ascontiguousarray(frames[0][sel, k]) for k in range(3))
    R = (_vdw(ubq.strings("element")[sel]) + np.float32(1.4)).astype(np.float32)
    _, buried = bc.split_counts(x, y, z, R, mask, sr.sphere_points(100))
    assert (buried > 0).sum() > 50 and (buried == 0).sum() > 50
    R6 = (_vdw(ubq.strings("element")[sel]) + np.float32(6.0)).astype(np.float32)
    assert (edge.neighbour_counts(x, y, z, R6) > 256).sum() > 100
    r = ensemble_check(bft, groups="C/H,L")
    fb = ens.jittered(bft, 1, seed=41)[0][r["atoms"]]
    R6 = (r["R"] - np.float32(1.4) + np.float32(6.0)).astype(np.float32)
    assert (edge.neighbour_counts(fb[:, 0], fb[:, 1], fb[:, 2], R6) > 256).sum() > 100
