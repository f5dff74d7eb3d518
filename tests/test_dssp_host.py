"""Secondary structure (arp_dssp) without a device: the host twin arp_dssp_host against pinned results, built helices and the numpy restatement of
tests/dssp_cases.py; chain breaks, chain starts and proline; tiny inputs, also under the address and undefined-behaviour sanitizers in a stand-alone program; the
input checks of arp_dssp (ctx == NULL); backbone_select.  Expected values never come from the call under test: they are pinned, derived in the docstrings, or
come from the restatement.
"""
from __future__ import annotations

import ctypes as C
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import arpeggia_amd as aa
import dssp_cases as dc
from arpeggia_amd import _lib
from arpeggia_amd import build as arp_build

ROOT = Path(__file__).resolve().parent.parent
H, B, E, G, I, T, S = (dc.SS.index(c) for c in "HBEGITS")
NONE = 0xFFFFFFFF


def twin(case: dict, flags=None) -> dict:
    return aa.secondary_structure_host(case["xyz"], case["flags"] if flags is None else flags)


def string(case: dict, flags=None) -> str:
    return aa.ss_string(twin(case, flags)["codes"][0])


def from_file(name: str):
    """(structure, selection, bb_xyz [1, R, 4, 3]) of a test file through the product's own loader and backbone_select."""
    s = aa.Structure.load(str(dc.DATA / name))
    sel = aa.backbone_select(s)
    soa = s.soa()
    xyz = np.stack([soa["x"], soa["y"], soa["z"]], 1)
    return s, sel, xyz[sel["bb"]][None]


def n_hbonds(res: dict) -> int:
    return int(((res["hb_acceptor"] != NONE) & (res["hb_energy"] < -0.5)).sum())


def test_margins_of_the_cases():
    """Every case of the device-equals-host comparison keeps 10^-6 from every threshold (asserted where they are built); the two files as the issue states."""
    cases = dc.device_cases()
    assert len(dc.SKIPPED_SEEDS) <= 1
    ubq, bft = (dc.margins(cases[k]["xyz"], cases[k]["flags"]) for k in ("1ubq", "6bft"))
    assert abs(ubq["E"] - 1.7e-3) < 1e-4 and abs(bft["E"] - 4.6e-4) < 1e-5, (ubq, bft)


def test_ubq_pinned():
    _, sel, x = from_file("1ubq.pdb")
    res = aa.secondary_structure_host(x, sel["flags"])
    assert aa.ss_string(res["codes"][0]) == dc.UBQ_STRING
    assert res["frame_counts"][0].tolist() == dc.UBQ_COUNTS
    assert res["counts"].sum(0).tolist() == dc.UBQ_COUNTS and (res["counts"].sum(1) == 1).all()
    assert n_hbonds(res) == dc.UBQ_HBONDS
    # the file's own HELIX records: H is exactly residues 23-34, G includes 57-59
    resi = [r for _, _, r in dc.pdb_case("1ubq.pdb")["res"]]
    assert [resi[k] for k in np.flatnonzero(res["codes"][0] == H)] == list(range(23, 35))
    assert {57, 58, 59} <= {resi[k] for k in np.flatnonzero(res["codes"][0] == G)}


def test_bft_pinned():
    _, sel, x = from_file("6bft.pdb")
    res = aa.secondary_structure_host(x, sel["flags"])
    assert res["frame_counts"][0].tolist() == dc.BFT_COUNTS
    assert n_hbonds(res) == dc.BFT_HBONDS


@pytest.mark.parametrize("name", ["1ubq.pdb", "6bft.pdb"])
def test_twin_against_the_restatement(name):
    """The twin's bonds and strands equal those of the numpy restatement, which shares no code with it."""
    case = dc.pdb_case(name)
    res = twin(case)
    got = {(int(a), j) for j in range(len(case["res"])) for a, e in zip(res["hb_acceptor"][0, j], res["hb_energy"][0, j]) if a != NONE and e < -0.5}
    assert got == dc.hbonds(case["xyz"][0], case["flags"])
    if name == "1ubq.pdb":   # (the restatement tries every pair in Python: the small file only)
        assert set(np.flatnonzero(res["codes"][0] == E).tolist()) == dc.bridges(case["xyz"][0], case["flags"])["E"]


def test_ideal_helices():
    """phi, psi = (-57, -47), (-49, -26), (-57, -70) as built (dssp_cases.HELIX_ANGLES) satisfy the energy criterion without adjustment: the restatement gives
    E(i, i + 4) = -2.22, E(i, i + 3) = -2.98 and E(i, i + 5) = -5.21 kcal/mol, every other E(i, i + n) of the three above -0.5."""
    R = dc.HELIX_RESIDUES
    for kind, n, code in (("alpha", 4, "H"), ("310", 3, "G"), ("pi", 5, "I")):
        case = dc.helix(kind)
        e = dc.geometry(case["xyz"][0], case["flags"])["E"]
        for m in (3, 4, 5):
            vals = [e[i, i + m] for i in range(R - m) if not np.isnan(e[i, i + m])]
            assert all(v < -1.0 for v in vals) if m == n else all(v > -0.5 for v in vals), (kind, m, vals)
        s = string(case)
        # turn_n(i) for i = 0 .. R - 1 - n, so the helix starts at i = 1 and its last start R - 1 - n ends at R - 2
        assert s[1 : R - 1] == code * (R - 2), (kind, s)
        assert set(s[0] + s[-1]) <= set("-T"), (kind, s)
        assert s.count(code) >= R - 4


def test_hairpin_fragment():
    """1ubq residues 1-17 on their own: the strand residues are the whole protein's, as far as both partners (and their neighbours) lie in the fragment."""
    ubq = dc.pdb_case("1ubq.pdb")
    frag = dc.fragment(ubq, lambda chain, resi: 1 <= resi <= 17)
    assert len(frag["res"]) == 17
    got = set(np.flatnonzero(twin(frag)["codes"][0] == E).tolist())
    want = dc.bridges(ubq["xyz"][0], ubq["flags"], inside=set(range(17)))["E"]
    assert got == want and len(want) >= 8
    whole = set(np.flatnonzero(twin(ubq)["codes"][0] == E).tolist())
    assert got <= whole and (whole - got) & set(range(17)) == {6}    # residue 7 pairs with the C-terminal strand only


def test_parallel_bridges_between_two_chains():
    """1ubq residues 1-7 as chain A and 64-72 as chain B: rows 0-6 and 7-15.  The restatement's bonds (acceptor, donor) are
    (3, 5), (3, 10), (5, 12), (8, 3), (10, 5), (11, 13), so by hand:
      par(3, 9):  hb(j-1, i) = (8, 3) and hb(i, j+1) = (3, 10)       par(4, 10): hb(i-1, j) = (3, 10) and hb(j, i+1) = (10, 5)
      par(5, 11): hb(j-1, i) = (10, 5) and hb(i, j+1) = (5, 12)
    three consecutive parallel bridges, a ladder: E on 3-5 and 9-11, nothing else (pinned from the twin after this check)."""
    ubq = dc.pdb_case("1ubq.pdb")
    rows = [k for k, (_, _, r) in enumerate(ubq["res"]) if 1 <= r <= 7 or 64 <= r <= 72]
    res = [(ubq["res"][k][0], "A" if ubq["res"][k][2] <= 7 else "B", ubq["res"][k][2]) for k in rows]
    case = dc.case_of(res, ubq["xyz"][:, rows])
    assert np.flatnonzero(case["flags"] & dc.CHAIN_START).tolist() == [0, 7]
    hb = dc.hbonds(case["xyz"][0], case["flags"])
    assert hb == {(3, 5), (3, 10), (5, 12), (8, 3), (10, 5), (11, 13)}
    assert {(8, 3), (3, 10)} <= hb and {(3, 10), (10, 5)} <= hb and {(10, 5), (5, 12)} <= hb
    found = dc.bridges(case["xyz"][0], case["flags"])
    assert found["par"] == {(3, 9), (4, 10), (5, 11), (9, 3), (10, 4), (11, 5)} and not found["anti"]
    assert string(case) == "---EEE---EEE----"


def test_gap_breaks_the_helix():
    """1ubq without residue 28: |C[27] - N[29]| > 2.5 is a break, no turn spans it, and the helix 23-34 falls into 23-26 and 29-33."""
    ubq = dc.pdb_case("1ubq.pdb")
    cut = dc.fragment(ubq, lambda chain, resi: resi != 28)
    at = {r: k for k, (_, _, r) in enumerate(cut["res"])}
    assert dc.geometry(cut["xyz"][0], cut["flags"])["brk"][at[29]] and not cut["flags"][at[29]] & dc.CHAIN_START
    res = twin(cut)
    code = res["codes"][0]
    assert not (code[at[27]] == H and code[at[29]] == H)
    runs = "".join("H" if c == H else "." for c in code).split(".")
    assert sorted(len(r) for r in runs if r) == [4, 5]
    assert aa.ss_string(code)[at[23] : at[34] + 1] == "HHHH--HHHHH"


def test_chain_start_splits_a_helix():
    """The 12-residue alpha helix with CHAIN_START on residue 6: two segments 0-5 and 6-11.  turn_4(i) needs cont(i, i + 4): i = 0, 1 and 6, 7, so H on
    1-4 and 7-10; 5 and 6 have no turn around them and no bend (cont(k - 2, k + 2) fails)."""
    case = dc.helix("alpha")
    assert string(case) == "-HHHHHHHHHH-"
    flags = case["flags"].copy()
    flags[6] |= dc.CHAIN_START
    assert string(case, flags) == "-HHHH--HHHH-"


def test_proline_donates_nothing():
    case = dc.helix("alpha")
    pro = dc.case_of([("PRO" if k == 6 else "ALA", "A", k + 1) for k in range(dc.HELIX_RESIDUES)], case["xyz"])
    assert pro["flags"][6] == dc.NO_H
    assert twin(case)["hb_acceptor"][0, 6, 0] == 2
    res = twin(pro)
    assert res["hb_acceptor"][0, 6].tolist() == [NONE, NONE] and res["hb_energy"][0, 6].tolist() == [0.0, 0.0]
    assert res["hb_acceptor"][0, 7, 0] == 3    # its neighbours keep theirs


def test_tiny_inputs_are_loop():
    ubq = dc.pdb_case("1ubq.pdb")
    for n in (1, 2, 3, 4, 5):
        res = twin(dc.first_residues(ubq, n))
        assert aa.ss_string(res["codes"][0]) == "-" * n
        assert res["counts"][:, 0].tolist() == [1] * n and res["frame_counts"][0].tolist() == [n] + [0] * 7


def test_tiny_inputs_under_sanitizers(tmp_path):
    """The host twin alone in a stand-alone program (tests/dssp_host), built with -fsanitize=address,undefined, on R = 1 .. 5 and the whole of 1ubq: every
    buffer is a heap block of exactly its size, so an access out of range ends the program."""
    ubq = dc.pdb_case("1ubq.pdb")
    cases = [dc.first_residues(ubq, n) for n in (1, 2, 3, 4, 5)] + [ubq]
    blob = struct.pack("<Q", len(cases))
    for c in cases:
        F, R = c["xyz"].shape[:2]
        blob += struct.pack("<QQ", F, R) + np.ascontiguousarray(c["xyz"], "<f8").tobytes() + c["flags"].tobytes()
    (tmp_path / "cases.bin").write_bytes(blob)
    prog = tmp_path / "dssp_host_main"
    subprocess.run([arp_build.hipcc(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "dssp_host" / "dssp_host_main.cpp"), "-o", str(prog)], check=True, capture_output=True)
    run = subprocess.run([str(prog), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout.split("\n")[:-1] == ["-", "--", "---", "----", "-----", dc.UBQ_STRING]


# ---- the input checks of arp_dssp, ctx == NULL -------------------------------------------------------------------------------------------------------------------------
def check_call(structure, frames, bb, flags, n_res=None):
    u8p, u32p, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    bb = np.ascontiguousarray(bb, "<u4")
    flags = np.ascontiguousarray(flags, "u1")
    n_frames, ptr = (0, None) if frames is None else (len(frames), np.ascontiguousarray(frames, "<f8").ctypes.data_as(dp))
    keep = (bb if bb.size else np.zeros(4, "<u4")), (flags if flags.size else np.zeros(1, "u1"))
    st = _lib.lib.arp_dssp(None, structure._h, n_frames, ptr, keep[0].ctypes.data_as(u32p), keep[1].ctypes.data_as(u8p), len(flags) if n_res is None else n_res,
                           None, None, None, None, None)
    return st, _lib.lib.arp_last_error().decode()


def test_input_errors():
    case = dc.helix("alpha")
    s = aa.Structure.from_records(dc.records(case))
    R = len(case["res"])
    bb, flags, frames = np.arange(4 * R).reshape(R, 4), case["flags"], dc.frames_of(case)
    assert check_call(s, frames, bb, flags)[0] == _lib.ARP_OK
    assert check_call(s, None, bb, flags)[0] == _lib.ARP_OK                     # the structure's one model
    st, msg = check_call(s, frames, bb[:0], flags[:0])
    assert st == _lib.ARP_ERR_BAD_INPUT and msg == "dssp: no residues (n_res == 0)"
    bad = bb.copy()
    bad[5, 2] = 4 * R
    st, msg = check_call(s, frames, bad, flags)
    assert st == _lib.ARP_ERR_BAD_INPUT and msg == f"dssp: bb[5][2] = {4 * R} is not an atom of the topology ({4 * R} atoms)"
    odd = flags.copy()
    odd[3] = 4
    st, msg = check_call(s, frames, bb, odd)
    assert st == _lib.ARP_ERR_BAD_INPUT and msg == "dssp: flags[3] = 4 has a bit other than CHAIN_START (1) and NO_H (2)"
    # the frame checks of the arp_rmsd_* calls, with their messages
    st, msg = check_call(s, frames[:0], bb, flags)
    assert st == _lib.ARP_ERR_BAD_INPUT and msg == "contact frequencies: at least one frame is needed"
    nan = np.repeat(frames, 2, 0)
    nan[1, 7, 1] = np.nan
    st, msg = check_call(s, nan, bb, flags)
    assert st == _lib.ARP_ERR_BAD_INPUT and msg == "contact frequencies: non-finite coordinate in frame 1, atom 7"
    with pytest.raises(aa.ArpeggiaError, match=r"dssp: frames must have shape \[F, 48, 3\]"):
        aa.api._secondary_structure(None, s, frames[:, :-1], "", True, False)
    # the twin's own
    with pytest.raises(aa.ArpeggiaError, match="dssp: flags\\[3\\] = 4"):
        aa.secondary_structure_host(case["xyz"], odd)
    with pytest.raises(aa.ArpeggiaError, match="dssp: at least one frame is needed"):
        aa.secondary_structure_host(case["xyz"][:0], flags)


# ---- backbone_select ---------------------------------------------------------------------------------------------------------------------------------------------
def test_backbone_select():
    s, sel, x = from_file("1ubq.pdb")
    assert len(sel["atom"]) == 76 and sel["bb"].shape == (76, 4) and sel["flags"].dtype == np.uint8
    assert np.flatnonzero(sel["flags"] & dc.CHAIN_START).tolist() == [0]
    names = s.strings("atomn")
    assert [names[k].decode() for k in sel["bb"][10]] == ["N", "CA", "C", "O"]
    ubq = dc.pdb_case("1ubq.pdb")
    assert np.array_equal(x[0], ubq["xyz"][0]) and np.array_equal(sel["flags"], ubq["flags"])   # the product's residues are the case file's
    assert {r for r, (n, _, _) in enumerate(ubq["res"]) if n == "PRO"} == set(np.flatnonzero(sel["flags"] & dc.NO_H).tolist()) != set()
    s6, sel6, x6 = from_file("6bft.pdb")
    assert len(sel6["atom"]) == dc.BFT_RESIDUES and int((sel6["flags"] & dc.CHAIN_START).sum()) == dc.BFT_CHAINS
    bft = dc.pdb_case("6bft.pdb")
    assert np.array_equal(x6[0], bft["xyz"][0]) and np.array_equal(sel6["flags"], bft["flags"])
    assert sorted({c for _, c, _ in bft["res"]}) == ["A", "B", "C", "G", "H", "L"]
    only = aa.backbone_select(s6, "H,L")
    assert {c.decode() for c in s6.strings("chain")[only["atom"]]} == {"H", "L"} and int((only["flags"] & dc.CHAIN_START).sum()) == 2


def test_backbone_select_drops_incomplete_residues():
    case = dc.helix("alpha")
    rec = dc.records(case)
    keep = np.ones(len(rec["x"]), bool)
    keep[4 * 5 + 3] = False                                 # residue 5 loses its O
    s = aa.Structure.from_records({k: v[keep] for k, v in rec.items()})
    sel = aa.backbone_select(s)
    assert len(sel["atom"]) == dc.HELIX_RESIDUES - 1
    assert s.ints("resi")[sel["atom"]].tolist() == [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]
    assert sel["bb"][5].tolist() == [23, 24, 25, 26]        # residue 7's atoms, one index down
    assert np.flatnonzero(sel["flags"] & dc.CHAIN_START).tolist() == [0]


def test_strings_and_table():
    assert aa.ss_string([0, 1, 2, 3, 4, 5, 6, 7]) == "-HBEGITS" == aa.SS_CODES
    counts = np.array([[1, 0, 0, 3, 0, 0, 0, 0], [2, 2, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 2, 2]])
    assert aa.ss_consensus(counts).tolist() == [3, 0, 6]      # the lower code on ties
    case = dc.helix("alpha")
    s = aa.Structure.from_records(dc.records(case))
    res = twin(case)
    res["residue"] = aa.backbone_select(s)["atom"]
    res["fraction"] = (res["counts"] / 1.0).astype("<f4")
    table = aa.secondary_structure_table(s, res)
    cols = {name: table[name].to_list() if hasattr(table[name], "to_list") else table[name].to_pylist() for name in aa.SS_COLUMNS}
    assert "".join(cols["consensus"]) == "-HHHHHHHHHH-" and cols["resi"] == list(range(1, 13)) and cols["frac_H"][1] == 1.0 and cols["frac_loop"][0] == 1.0
