"""RMSD between frames: everything that needs no device.  arp_rmsd_host (the definition in plain sequential C++, the yardstick of k_rmsd_pack / k_rmsd_gram /
k_rmsd_to_centre) against the numpy reference on every case, within the derived bound; the reference against an independent f64 route; every input check of
the three device calls with ctx == NULL; rmsd_select; the cases' reach; the cluster fixture's separation; the exports and the CLI's flags."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import rmsd_cases as rc
from arpeggia_amd import _lib
from arpeggia_amd._lib import lib


def refused(status: int, fn, *args, match: str | None = None, **kw):
    with pytest.raises(aa.ArpeggiaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)
    return str(e.value)


def test_exported():
    header = (Path(aa.__file__).resolve().parent.parent / "include" / "arpeggia_amd.h").read_text()
    for name in ("arp_rmsd_matrix", "arp_rmsd_reference", "arp_rmsd_clusters", "arp_rmsd_host"):
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\(", header), name
    assert lib.arp_api_version() == 2  # additive exports do not move the layout version
    for word in ("rmsd_cap_bytes", "rmsd_chunk_atoms", "rmsd_to_centre", "Horn", "proper rotations", "strictly increasing", "gromos"):
        assert word in header, word
    for name in ("rmsd_select", "rmsd_host", "get_rmsd", "get_rmsd_matrix", "get_rmsd_clusters", "rmsd", "rmsd_matrix", "rmsd_clusters"):
        assert callable(getattr(aa, name))
    for name in ("rmsd", "rmsd_matrix", "rmsd_clusters"):
        assert callable(getattr(aa.Context, name))


def test_cases_reach_their_mechanisms():
    rc.check_shape_reach()
    rc.check_degenerate_reach()


def test_cluster_fixture_is_separated():
    """Measured on the reference: within a state at most 0.42 A, between states at least 3.30 A; no pair within the bound of the 1.0 A cutoff."""
    got = rc.check_cluster_fixture()
    print(f"cluster fixture: within {got['within']:.4f} A, between {got['between']:.4f} A")


def test_reference_by_hand():
    """The numpy reference itself on frames small enough to do by hand."""
    a = np.array([[0.0, 0, 0], [2.0, 0, 0]])
    frames = np.stack([a, a + 5.0, a[:, [1, 0, 2]], a * 2.0])   # translated, turned by 90 degrees, stretched: centred x = -1, 1 against -2, 2
    r = rc.reference(frames)
    assert r["rmsd"][0, 1] == 0.0 and abs(r["rmsd"][0, 2]) < 1e-7 and abs(r["rmsd"][0, 3] - 1.0) < 1e-12
    # a chiral tetrahedron and its mirror image: the best proper rotation leaves a residual, the SVD without the determinant sign would give 0
    t = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0], [0, 0, 3.0]])
    m = rc.reference(np.stack([t, rc.mirror(t)]))["rmsd"]
    assert m[0, 1] > 0.3
    assert np.allclose(rc.horn_eigvalsh(np.stack([t, rc.mirror(t)])), m, atol=1e-12)


def test_reference_against_an_independent_route():
    """SVD-Kabsch and eigvalsh of Horn's K, both f64, agree far inside the bound on every case: the reference alone does not use the bound up."""
    worst = 0.0
    cases = dict(rc.degenerate_cases(), synthetic=rc.synthetic(17, 65), fixture=rc.cluster_fixture()[0][:20])
    for name, X in cases.items():
        worst = max(worst, rc.assert_within(rc.horn_eigvalsh(X), rc.reference(X), name))
    print(f"largest |svd - eigvalsh| / bound: {worst:.4f}")
    assert worst <= 0.25


@pytest.mark.parametrize("F", rc.CHEAP_FRAMES)
def test_host_shapes(F):
    for n in rc.ATOMS:
        X = rc.synthetic(F, n)
        got = aa.rmsd_host(X)
        assert got.dtype == np.float32 and got.shape == (F, F)
        assert np.array_equal(got, got.T) and (np.diag(got) == 0).all()
        rc.assert_within(got, rc.reference(X), (F, n))
        if n == 1:
            assert (got == 0).all()


def test_host_degenerate():
    for name, X in rc.degenerate_cases().items():
        got = aa.rmsd_host(X)
        rc.assert_within(got, rc.reference(X), name)
        assert np.array_equal(got, got.T), name
    m = aa.rmsd_host(rc.degenerate_cases()["mirror"])
    assert m[0, 1] > 1.0


def test_host_fixture():
    frames, _ = rc.cluster_fixture()
    got = aa.rmsd_host(frames)
    rc.assert_within(got, rc.reference(frames), "fixture")
    mine, want = rc.clusters(got, rc.CLUSTER_CUTOFF), rc.check_cluster_fixture()["want"]
    for key in ("cluster", "n_neighbours", "centre", "cluster_size"):   # (rmsd_to_centre: f32 values of two f64 routes, equal within the bound only)
        assert np.array_equal(mine[key], want[key]), key


def test_host_refusals():
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsd_host, np.zeros((2, 0, 3)), match="empty")
    x = np.zeros((2, 3, 3))
    x[1, 2, 0] = np.inf
    refused(_lib.ARP_ERR_BAD_INPUT, aa.rmsd_host, x, match="frame 1, atom 2")
    with pytest.raises(ValueError):
        aa.rmsd_host(np.zeros((2, 3)))
    assert aa.rmsd_host(np.zeros((0, 4, 3))).shape == (0, 0)


# ---- rmsd_select ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


def test_select_on_1ubq(ubq):
    for atoms, count in (("ca", 76), ("heavy", 602), ("backbone", 304), ("all", 602)):
        got = aa.rmsd_select(ubq, atoms)
        assert got.dtype == np.dtype("<u4") and np.array_equal(got, rc.ubq_selection(atoms)) and len(got) == count, atoms
    assert len(rc.ubq_atoms()) > 602  # the file has waters: HOH is left out of every keyword
    assert np.array_equal(aa.rmsd_select(ubq), aa.rmsd_select(ubq, "ca"))
    assert np.array_equal(aa.rmsd_select(ubq, "ca", "A"), aa.rmsd_select(ubq, "ca")) and np.array_equal(aa.rmsd_select(ubq, "ca", "A, B"), aa.rmsd_select(ubq, "ca"))
    assert len(aa.rmsd_select(ubq, "ca", "B")) == 0
    with pytest.raises(ValueError):
        aa.rmsd_select(ubq, "sidechain")


def test_select_explicit_arrays(ubq):
    assert aa.rmsd_select(ubq, [5, 3, 9]).tolist() == [3, 5, 9] and aa.rmsd_select(ubq, np.array([7], np.int64)).dtype == np.dtype("<u4")
    with pytest.raises(ValueError, match="duplicate"):
        aa.rmsd_select(ubq, [3, 5, 3])
    with pytest.raises(ValueError):
        aa.rmsd_select(ubq, [-1, 2])
    with pytest.raises(ValueError):
        aa.rmsd_select(ubq, [0.5, 2.0])
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd_matrix, ubq, frames_of(ubq, 2), atoms=[0, 10 ** 6], match="not an atom of the topology")


# ---- what the three calls decide before the device is touched ------------------------------------------------------------------------------------------------
def frames_of(s: aa.Structure, F: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"], soa["y"], soa["z"]], 1)[None].repeat(F, 0)


def raw(s, frames, sel, call="matrix", ref=None, ref_frame=0, cutoff=1.0, cap=_lib.ARP_NONE) -> tuple:
    """The ABI call with ctx == NULL: (status, message)."""
    n_frames, ptr, keep = aa.api._frames_arg(s, frames, "rmsd")
    sel = np.ascontiguousarray(sel, "<u4")
    sp = (sel if len(sel) else np.zeros(1, "<u4")).ctypes.data_as(C.POINTER(C.c_uint32))
    if call == "matrix":
        st = lib.arp_rmsd_matrix(None, s._h, int(n_frames), ptr, sp, len(sel), None)
    elif call == "reference":
        rp = None if ref is None else np.ascontiguousarray(ref, "<f8").ctypes.data_as(C.POINTER(C.c_double))
        st = lib.arp_rmsd_reference(None, s._h, int(n_frames), ptr, sp, len(sel), rp, int(ref_frame), None)
    else:
        st = lib.arp_rmsd_clusters(None, s._h, int(n_frames), ptr, sp, len(sel), C.c_float(cutoff), cap, *([None] * 6))
    return st, lib.arp_last_error().decode()


CALLS = ("matrix", "reference", "clusters")


def test_null_context_runs_only_the_checks(ubq):
    f = frames_of(ubq, 3)
    for call in CALLS:
        assert raw(ubq, f, [0, 5, 9], call)[0] == _lib.ARP_OK
        assert raw(ubq, None, [0], call)[0] == _lib.ARP_OK   # the structure's one model is the one frame
    assert raw(ubq, f, [1, 2], "reference", ref_frame=2)[0] == _lib.ARP_OK
    assert raw(ubq, f, [1, 2], "reference", ref=f[0], ref_frame=99)[0] == _lib.ARP_OK   # ref_frame is not looked at next to ref_xyz
    assert raw(ubq, f, [1, 2], "clusters", cutoff=0.0, cap=1)[0] == _lib.ARP_OK


@pytest.mark.parametrize("call", CALLS)
def test_selection_checks(ubq, call):
    f = frames_of(ubq, 2)
    N = f.shape[1]
    for sel, words in (([], "selection is empty"), ([0, N], "not an atom of the topology"), ([3, 3], "not strictly increasing"), ([5, 4], "not strictly increasing")):
        st, msg = raw(ubq, f, sel, call)
        assert st == _lib.ARP_ERR_BAD_INPUT and words in msg and msg.startswith("rmsd "), (sel, msg)


@pytest.mark.parametrize("call", CALLS)
def test_frame_checks_are_those_of_the_frequency_call(ubq, call):
    """Same statuses and messages, and they come before the call's own checks."""
    def freq(frames):
        n_frames, ptr, keep = aa.api._frames_arg(ubq, frames, "contact frequencies")
        t = C.c_void_p()
        return lib.arp_contact_frequencies(None, ubq._h, int(n_frames), ptr, b"/", 0.1, 6.5, C.byref(t)), lib.arp_last_error().decode()

    bad = frames_of(ubq, 3)
    bad[2, 17, 1] = np.nan
    for frames, words in ((frames_of(ubq, 0), "at least one frame"), (bad, "frame 2, atom 17")):
        want = freq(frames)
        assert want[0] == _lib.ARP_ERR_BAD_INPUT and words in want[1]
        assert raw(ubq, frames, [], call, ref_frame=99, cutoff=-1.0, cap=0) == want


def test_reference_checks(ubq):
    f = frames_of(ubq, 3)
    st, msg = raw(ubq, f, [0, 1], "reference", ref_frame=3)
    assert st == _lib.ARP_ERR_BAD_INPUT and msg.startswith("rmsd reference: ref_frame 3")
    ref = f[0].copy()
    ref[11, 2] = np.inf
    st, msg = raw(ubq, f, [0, 1], "reference", ref=ref)
    assert st == _lib.ARP_ERR_BAD_INPUT and "non-finite coordinate in ref_xyz, atom 11" in msg
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd, ubq, f, reference=np.zeros((4, 3)), match="shape")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd, ubq, f, reference=7, match="ref_frame 7")
    with pytest.raises(ValueError):
        aa.get_rmsd(ubq, f, reference=-1)


@pytest.mark.parametrize("cutoff", [float("nan"), float("inf"), -0.5])
def test_bad_cutoff(ubq, cutoff):
    st, msg = raw(ubq, frames_of(ubq, 2), [0, 1], "clusters", cutoff=cutoff)
    assert st == _lib.ARP_ERR_BAD_INPUT and msg.startswith("rmsd clusters: cutoff")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd_clusters, ubq, frames_of(ubq, 2), cutoff=cutoff, match="cutoff")


def test_bad_max_clusters_and_missing_cutoff(ubq):
    st, msg = raw(ubq, frames_of(ubq, 2), [0, 1], "clusters", cap=0)
    assert st == _lib.ARP_ERR_BAD_INPUT and "max_clusters" in msg
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd_clusters, ubq, frames_of(ubq, 2), cutoff=1.0, max_clusters=0, match="max_clusters")
    with pytest.raises(ValueError):
        aa.get_rmsd_clusters(ubq, frames_of(ubq, 1), cutoff=1.0, max_clusters=-3)
    for fn, args in ((aa.get_rmsd_clusters, (ubq,)), (aa.rmsd_clusters, ("x.pdb",)), (aa.Context.rmsd_clusters, (None, ubq))):
        with pytest.raises(TypeError):
            fn(*args)  # cutoff has no default in any layer


def test_input_errors_come_before_the_missing_device(ubq):
    """Whatever the machine: a bad input is ARP_ERR_BAD_INPUT from every layer, never ARP_ERR_NO_DEVICE."""
    f = frames_of(ubq, 2)
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd, ubq, f, atoms="ca", chains="Z", match="selection is empty")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd_matrix, ubq, np.zeros((2, 5, 3)), match="shape")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd_matrix, ubq, frames_of(ubq, 0), match="at least one frame")
    refused(_lib.ARP_ERR_BAD_INPUT, aa.get_rmsd_clusters, ubq, f, atoms=[0, 10 ** 6], cutoff=1.0, match="not an atom")


def test_knobs():
    for knob in ("rmsd_cap_bytes", "rmsd_chunk_atoms"):
        aa.debug_set(knob, 1)
        aa.debug_set(knob, 1 << 40)
        aa.debug_set(knob, 0)
        refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, knob, -1)
        assert knob in refused(_lib.ARP_ERR_BAD_INPUT, aa.debug_set, "no_such_knob", 1)


def test_ten_to_the_five_frames_are_legal_for_the_cluster_call_by_the_arithmetic():
    F, n_pad = 10 ** 5, 76
    assert F * -(-F // 32) * 4 == 1_250_000_000 < 2 ** 31 < F * F * 4 and F * 3 * n_pad * 8 + F * 8 < 2 ** 31


def test_cli_defaults_and_flags(tmp_path):
    from arpeggia_amd.__main__ import build_parser

    p = build_parser()
    a = p.parse_args(["rmsd", "-i", "x.pdb", "-o", str(tmp_path)])
    assert a.reference == 0 and a.atoms == "ca" and a.chains == ""
    a = p.parse_args(["rmsd", "-i", "x.pdb", "-o", str(tmp_path), "--reference", "3", "--atoms", "backbone", "-c", "A,B"])
    assert a.reference == 3 and a.atoms == "backbone" and a.chains == "A,B"
    a = p.parse_args(["rmsd-matrix", "-i", "x.pdb", "--matrix", str(tmp_path / "m.npy"), "--atoms", "heavy"])
    assert str(a.matrix).endswith("m.npy") and a.atoms == "heavy"
    a = p.parse_args(["rmsd-clusters", "-i", "x.pdb", "-o", str(tmp_path), "--cutoff", "1.5"])
    assert a.cutoff == 1.5 and a.max_clusters is None and a.assignments is None
    a = p.parse_args(["rmsd-clusters", "-i", "x.pdb", "-o", str(tmp_path), "--cutoff", "2", "--max-clusters", "4", "--assignments", "a.csv"])
    assert a.max_clusters == 4 and str(a.assignments) == "a.csv"
    for argv in (["rmsd-clusters", "-i", "x.pdb", "-o", str(tmp_path)], ["rmsd", "-i", "x.pdb", "-o", str(tmp_path), "--atoms", "sidechain"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
