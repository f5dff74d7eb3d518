"""Water bridges on the device: ARP_FREQ_WATERS on the residue frequency call and the timeline call, and arp_water_bridges (freq_water.inl).

Expected values come from tests/water_bridge_restatement.py (plain numpy on the topology's SoA columns and the frames) and, for the built cases of
tests/water_bridge_cases.py, from their closed form as well; tests/test_water_bridge_host.py pins the two to each other on the CPU.  The rows of the
other interactions are compared with the same call without the flag, byte for byte.  Expected values never come from the calls under test."""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import freq_residue_common as fc
import water_bridge_cases as wc
import water_bridge_restatement as wr
from arpeggia_amd import _lib

pytestmark = pytest.mark.gpu

KNOBS = ("freq_chunk_atoms", "freq_cap_items", "freq_frame_bits")
HOWS = ("one_pass", "three_passes", "cap_1", "frame_bits_2")
UBQ_COUNTS = (21, 20, 4)  # 1ubq as one frame: triples, residue rows, most partners of one water (test_water_bridge_host.py pins them to the restatement)


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    for k in KNOBS:
        aa.debug_set(k, 0)


def knobs(how: str, F: int, n: int):
    values = {"one_pass": (0, 0, 0), "three_passes": (-(-F // 3) * n, 0, 0), "cap_1": (0, 1, 0), "frame_bits_2": (0, 0, 2)}[how]
    for k, v in zip(KNOBS, values):
        aa.debug_set(k, v)


@pytest.fixture(scope="module")
def ubq(ubq_path):
    """1ubq, its crystal coordinates as one frame, and 16 jittered frames (seeded, sigma 0.3 A), with the restatement of both."""
    s = aa.load_model(ubq_path)
    soa = s.soa("/")
    one = np.stack([soa["x"], soa["y"], soa["z"]], axis=1)[None].copy()
    jit = one + np.random.default_rng(30).normal(0.0, 0.3, (16,) + one.shape[1:])
    out = {"s": s, "one": one, "jitter": jit}
    for k in ("one", "jitter"):
        stats = {}
        out[k + "_triples"] = wr.triples(s, out[k], "/", stats)
        out[k + "_stats"] = stats
        out[k + "_rows"] = wr.residue_rows(s, out[k], "/")
    return out


def water_rows(t: dict) -> dict:
    sel = t["interaction"] == wr.CODE
    return {c: t[c][sel] for c in fc.COLUMNS}


def other_rows(t: dict) -> dict:
    sel = t["interaction"] != wr.CODE
    return {c: t[c][sel] for c in fc.COLUMNS}


def expect_capacity(call):
    with pytest.raises(aa.ArpeggiaError) as e:
        call()
    assert e.value.status == _lib.ARP_ERR_CAPACITY and "32 polar atoms" in str(e.value)


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", list(wc.cases()))
def test_built_cases(ctx, name, how):
    """legs: the inclusive 3.5 A edge, one ulp either side.  separation: same residue, ord + 1, + 2, + 3, one orientation, two atom pairs of one residue
    pair.  chains[*]: orientation by the groups, the dedupe of chains in both sets, a partner without a bit.  third_chain_no_pair: a pass without any
    atom pair still yields the row.  two_waters: a frame counts once, the closest approach is the tighter bridge.  schedule70: forms, breaks, re-forms
    over 3 bitmap words.  waters_63/64/65, polars_255/256/257: the tile edge and the sweep step, the bridge at the last index.  partners_32/33: the full
    list, and one too many -- a status, no table.  Each in one pass, in three, with buffers of one item and with two frame bits."""
    wc.check_reach(name)
    c = wc.cases()[name]
    s = aa.Structure.from_records(c.rec)
    assert s.n_atoms == c.n
    knobs(how, c.F, c.n)
    call = lambda waters: ctx.contact_frequencies(s, c.frames, c.groups, level="residue", waters=waters)
    off = call(False)
    if c.capacity:
        expect_capacity(lambda: call(True))
        expect_capacity(lambda: ctx.contact_timelines(s, c.frames, c.groups, level="residue", waters=True))
        expect_capacity(lambda: ctx.water_bridges(s, c.frames, c.groups))
        return
    got = call(True)
    fc.assert_same_table(water_rows(got), wc.expected_rows(c))                      # the closed form
    fc.assert_same_table(got, wr.merge(off, wr.residue_rows(s, c.frames, c.groups)))  # the restatement, among the flag-off rows in key order
    assert fc.to_bytes(call(True)) == fc.to_bytes(got)
    if name == "third_chain_no_pair":
        assert len(off["n_frames"]) == 0 and len(got["n_frames"]) == 1  # no atom pair in the whole pass
    if name == "partners_32":
        assert len(got["n_frames"][got["interaction"] == wr.CODE]) == 256


@pytest.mark.parametrize("rings", [False, True])
@pytest.mark.parametrize("frames", ["one", "jitter"])
def test_ubq_table_and_the_other_rows(ctx, ubq, frames, rings):
    """1ubq as one frame and x 16 jittered frames: the water rows equal the restatement, every other row is byte for byte the flag-off table's, with
    and without ring rows, and the rows are in key order."""
    s, xyz = ubq["s"], ubq[frames]
    off = ctx.contact_frequencies(s, xyz, "/", rings=rings, level="residue")
    got = ctx.contact_frequencies(s, xyz, "/", rings=rings, level="residue", waters=True)
    assert fc.to_bytes(other_rows(got)) == fc.to_bytes(off)
    fc.assert_same_table(water_rows(got), ubq[frames + "_rows"])
    fc.assert_same_table(got, wr.merge(off, ubq[frames + "_rows"]))
    assert fc.to_bytes(ctx.contact_frequencies(s, xyz, "/", rings=rings, level="residue", waters=True)) == fc.to_bytes(got)
    if frames == "one":
        assert (len(ubq["one_triples"]), int((got["interaction"] == wr.CODE).sum()), ubq["one_stats"]["max_partners"]) == UBQ_COUNTS
    else:
        assert len(ubq["jitter_triples"]) > 0 and ubq["jitter_stats"]["max_partners"] <= wc.PARTNERS
        aa.debug_set("freq_chunk_atoms", 6 * xyz.shape[1])  # three passes
        aa.debug_set("freq_cap_items", 1)
        assert fc.to_bytes(ctx.contact_frequencies(s, xyz, "/", rings=rings, level="residue", waters=True)) == fc.to_bytes(got)


def check_timeline(tl: dict, freq: dict, pres: dict, F: int):
    assert all(np.array_equal(tl[c], freq[c]) for c in fc.COLUMNS)
    bits = aa.unpack_timeline(tl["timeline_words"], F)
    assert tl["n_total_frames"] == F and np.array_equal(bits.sum(axis=1), tl["n_frames"])  # the popcount
    rows = np.flatnonzero(tl["interaction"] == wr.CODE)
    assert len(rows) == len(pres)
    for r in rows:
        assert np.array_equal(bits[r], pres[(int(tl["from_residue"][r]), int(tl["to_residue"][r]))])
    host = aa.timeline_stats(tl["timeline_words"], F)
    for c in ("first_frame", "last_frame", "n_events", "longest_run"):
        assert np.array_equal(tl[c], host[c]), c


@pytest.mark.parametrize("how", ["one_pass", "three_passes", "cap_1"])
@pytest.mark.parametrize("name", ["legs", "two_waters", "schedule70", "third_chain_no_pair", "waters_65", "partners_32"])
def test_timelines_of_built_cases(ctx, name, how):
    c = wc.cases()[name]
    s = aa.Structure.from_records(c.rec)
    knobs(how, c.F, c.n)
    freq = ctx.contact_frequencies(s, c.frames, c.groups, level="residue", waters=True)
    tl = ctx.contact_timelines(s, c.frames, c.groups, level="residue", waters=True)
    check_timeline(tl, freq, wc.expected_presence(c), c.F)
    if c.timeline:
        r = int(np.flatnonzero(tl["interaction"] == wr.CODE)[0])
        assert tl["timeline_words"].shape[1] == 3
        assert {k: int(tl[k][r]) for k in c.timeline} == c.timeline
    none = ctx.contact_timelines(s, c.frames, c.groups, level="residue", waters=True, bitmap=False)
    assert "timeline_words" not in none and all(np.array_equal(none[k], tl[k]) for k in none)


@pytest.mark.parametrize("rings", [False, True])
def test_timelines_of_ubq(ctx, ubq, rings):
    s, xyz = ubq["s"], ubq["jitter"]
    freq = ctx.contact_frequencies(s, xyz, "/", rings=rings, level="residue", waters=True)
    tl = ctx.contact_timelines(s, xyz, "/", rings=rings, level="residue", waters=True)
    check_timeline(tl, freq, wr.presence(s, xyz, "/"), xyz.shape[0])
    off = ctx.contact_timelines(s, xyz, "/", rings=rings, level="residue")
    sel = tl["interaction"] != wr.CODE
    assert all(np.array_equal(tl[k][sel], off[k]) for k in off if k != "n_total_frames")


def check_triples(ctx, s, frames, groups, want: np.ndarray):
    got = ctx.water_bridges(s, frames, groups)
    assert set(got) == {c for c, _ in aa.WATER_BRIDGE_COLUMNS} | {"from_atom", "water_atom", "to_atom"}
    for col, key in (("frame", "frame"), ("from_atom", "p"), ("to_atom", "q"), ("water_atom", "w")):
        assert np.array_equal(got[col], want[key].astype(got[col].dtype)), col
    for col, key in (("from_distance", "dp"), ("to_distance", "dq")):
        assert got[col].dtype == np.float32 and np.array_equal(got[col].view(np.uint32), want[key].view(np.uint32)), col
    assert np.array_equal(got["distance"], np.maximum(want["dp"], want["dq"]))
    n = np.asarray(frames).shape[1]
    for side, atom in (("from", got["from_atom"]), ("to", got["to_atom"]), ("water", got["water_atom"])):
        assert np.array_equal(got[f"{side}_chain"], s.strings("chain")[:n][atom]) and np.array_equal(got[f"{side}_resi"], s.ints("resi")[:n][atom])
        assert np.array_equal(got[f"{side}_atomi"], s.ints("atomi")[:n][atom]) and np.array_equal(got[f"{side}_altloc"], s.strings("altloc")[:n][atom])
        if side != "water":
            assert np.array_equal(got[f"{side}_resn"], s.strings("resn")[:n][atom]) and np.array_equal(got[f"{side}_atomn"], s.strings("atomn")[:n][atom])
    assert (s.strings("resn")[:n][got["water_atom"]] == b"HOH").all()
    return got


@pytest.mark.parametrize("how", ["one_pass", "three_passes", "cap_1"])
@pytest.mark.parametrize("name", [n for n, c in wc.cases().items() if not c.capacity])
def test_water_bridges_of_built_cases(ctx, name, how):
    c = wc.cases()[name]
    s = aa.Structure.from_records(c.rec)
    knobs(how, c.F, c.n)
    want = wc.expected_triples(c)
    got = check_triples(ctx, s, c.frames, c.groups, np.rec.fromarrays([want[k] for k in ("frame", "p", "q", "w", "dp", "dq")], names="frame,p,q,w,dp,dq"))
    assert np.array_equal(got["frame"], wr.triples(s, c.frames, c.groups)["frame"])
    again = ctx.water_bridges(s, c.frames, c.groups)
    assert fc.to_bytes(again) == fc.to_bytes(got)


@pytest.mark.parametrize("frames", ["one", "jitter"])
def test_water_bridges_of_ubq(ctx, ubq, frames):
    """The rows equal the restatement's triples, and grouping them by residue reproduces the frequency call's WaterBridge rows exactly."""
    s, xyz = ubq["s"], ubq[frames]
    got = check_triples(ctx, s, xyz, "/", ubq[frames + "_triples"])
    res = s.soa("/")["res_id"][: xyz.shape[1]].astype(np.int64)
    grouped = fc.group_by_residue(s, xyz.shape[0], xyz.shape[1], res[got["from_atom"]], res[got["to_atom"]], np.full(len(got["frame"]), wr.CODE, np.int64),
                                  got["frame"].astype(np.int64), got["distance"])
    freq = ctx.contact_frequencies(s, xyz, "/", level="residue", waters=True)
    fc.assert_same_table(water_rows(freq), grouped)
    aa.debug_set("freq_chunk_atoms", 5 * xyz.shape[1])
    aa.debug_set("freq_cap_items", 3)
    assert fc.to_bytes(ctx.water_bridges(s, xyz, "/")) == fc.to_bytes(got)


def test_module_level_calls_and_arrow(ubq, ubq_path):
    t = aa.get_contact_frequencies(ubq["s"], ubq["one"], level="residue", waters=True)
    arrow = t if hasattr(t, "column") and not hasattr(t, "to_arrow") else t.to_arrow()
    names = arrow.column("interaction").to_pylist()
    assert names.count("WaterBridge") == UBQ_COUNTS[1] and "?" not in names
    b = aa.water_bridges(ubq_path)
    arrow = b if hasattr(b, "column") and not hasattr(b, "to_arrow") else b.to_arrow()
    assert arrow.column_names == [c for c, _ in aa.WATER_BRIDGE_COLUMNS] and arrow.num_rows == UBQ_COUNTS[0]
    tl = aa.get_contact_timelines(ubq["s"], ubq["one"], level="residue", waters=True)
    assert int((tl["interaction"] == wr.CODE).sum()) == UBQ_COUNTS[1]


def test_cli(ubq_path, tmp_path):
    from arpeggia_amd.__main__ import main

    assert main(["contact-frequency", "-i", ubq_path, "-o", str(tmp_path), "-l", "residue", "--waters"]) == 0
    assert main(["contact-timeline", "-i", ubq_path, "-o", str(tmp_path), "-l", "residue", "--waters", "--rings"]) == 0
    assert main(["water-bridges", "-i", ubq_path, "-o", str(tmp_path), "-g", "/", "-t", "csv"]) == 0
    for name in ("contact_frequency.csv", "contact_timeline.csv"):
        lines = (tmp_path / name).read_text().splitlines()
        assert sum("WaterBridge" in ln for ln in lines) == UBQ_COUNTS[1], name
    lines = (tmp_path / "water_bridges.csv").read_text().splitlines()
    assert [h.strip('"') for h in lines[0].split(",")] == [c for c, _ in aa.WATER_BRIDGE_COLUMNS] and len(lines) == 1 + UBQ_COUNTS[0]
