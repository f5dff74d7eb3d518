"""The ring rules at their thresholds on the device: the table path (k_fit_planes, k_ring_atom, k_ring_ring of table_dev.hip) and the frame path
(k_freq_ring_fit, k_freq_ring_rows of freq_rings.inl) on the built cases of tests/ring_edge_rules.py.

tests/test_ring_edge_host.py holds the restatement to the oracle on the CPU; here the device is held to both, with no tolerance anywhere:
  planes   arp_structure_fit_planes: the exact-plane rings are the closed form bit for bit, every other ring is the Python port of the fit bit
           for bit (every operation of the fit is IEEE and the build does not contract)
  table    get_contacts per family: the ring rows (from entity, to entity, code, f32 distance bits) are the restatement on the device's own
           planes and, for the exact-plane families, the oracle's rows; the atom rows of the same call are the oracle's
           -- except, for the tilted rings, at the points where the restatement itself differs between the oracle's planes and the device's
  frames   arp_contact_timelines with ARP_FREQ_RINGS per sweep, a frame per sweep point: present[row][frame] and the rows' smallest and largest
           distance are the restatement's (on the closed-form planes, or on the ported fit's), in one pass and in two, and once at the residue level
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import arpeggia_amd as aa
import oracle_binding as ob
import ring_edge_rules as R
import synth
from arpeggia_amd import _lib

pytestmark = pytest.mark.gpu

EXACT = ("a", "b", "c", "f3", "f4")
RING_CODES = set(range(11, 18))


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    aa.debug_set("freq_chunk_atoms", 0)


def bits64(v) -> tuple:
    return tuple(np.asarray(v, dtype="<f8").view(np.uint64).tolist())


def device_planes(ctx, s, top: R.Topology) -> dict:
    nres = int(_lib.lib.arp_structure_n_residues(s._h))
    assert nres == len(top.res_key)
    planes, valid = np.zeros((nres, 12)), np.zeros(nres, dtype=np.uint8)
    st = _lib.lib.arp_structure_fit_planes(ctx._h, s._h, planes.ctypes.data_as(C.POINTER(C.c_double)), valid.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert st == 0, _lib.lib.arp_last_error()
    assert [bool(v & 1) for v in valid] == [bool(ra) for ra in top.ring_atoms]
    return {r: R.Plane(tuple(planes[r, 0:3].tolist()), tuple(planes[r, 3:6].tolist())) for r in range(nres) if valid[r] & 1}


def device_rows(ctx, s, top: R.Topology, cutoff: float):
    """(ring rows, atom rows) of one get_contacts call as sets of (from entity, to entity, code, f32 distance bits)."""
    t = ctx.get_contacts(s, "/", 0.1, cutoff)
    ent = {(top.res_key[r][0], top.res_key[r][1], alt): e for e, (r, alt) in enumerate(top.rings)}
    d = np.ascontiguousarray(t["distance"], dtype="<f4").view(np.uint32)
    ring, atom = [], []
    for k in range(len(d)):
        code, fa, ta = int(t["interaction"][k]), int(t["from_atom"][k]), int(t["to_atom"][k])
        if fa >= 0:
            assert ta >= 0 and code not in RING_CODES
            atom.append((fa, ta, code, int(d[k])))
            continue
        assert code in RING_CODES and t["from_atomn"][k] == b"Ring"
        frm = top.n + ent[(bytes(t["from_chain"][k]), int(t["from_resi"][k]), bytes(t["from_altloc"][k]))]
        to = ta if ta >= 0 else top.n + ent[(bytes(t["to_chain"][k]), int(t["to_resi"][k]), bytes(t["to_altloc"][k]))]
        ring.append((frm, to, code, int(d[k])))
    assert len(set(ring)) == len(ring) and len(set(atom)) == len(atom)
    return set(ring), set(atom)


def oracle_rows(top: R.Topology, rec, cutoff: float):
    orc = ob.Structure.from_atoms(synth.records_to_oracle(rec, flat=False), flat=False)
    ent = {(top.res_key[r][0], top.res_key[r][1], alt): e for e, (r, alt) in enumerate(top.rings)}
    ring, atom = set(), set()
    for r in orc.get_contacts("/", 0.1, cutoff):
        code, dist = int(r["interaction"]), int(np.float32(r["distance"]).view(np.uint32))
        if int(r["from_atom"]) >= 0:
            atom.add((int(r["from_atom"]), int(r["to_atom"]), code, dist))
            continue
        f, t = r["from"], r["to"]
        frm = top.n + ent[(bytes(f["chain"]), int(f["resi"]), bytes(f["altloc"]))]
        to = int(r["to_atom"]) if int(r["to_atom"]) >= 0 else top.n + ent[(bytes(t["chain"]), int(t["resi"]), bytes(t["altloc"]))]
        ring.add((frm, to, code, dist))
    return ring, atom


def describe(b: R.Built, fam: str, rows) -> list:
    """The sweeps and points that a set of differing rows belongs to (for the failure message)."""
    ent_res = [r for r, _ in b.top.rings]
    sw = R.sweeps(fam)
    return sorted({(sw[b.motifs[ent_res[x[0] - b.top.n]][0]].label, b.motifs[ent_res[x[0] - b.top.n]][1]) for x in rows if ent_res[x[0] - b.top.n] < len(b.motifs)})


# ---- planes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_planes(ctx, fam):
    b = R.structure(fam)
    got = device_planes(ctx, aa.Structure.from_records(b.rec), b.top)
    port = R.port_planes(b.top, b.xyz)
    assert set(got) == set(port)
    for r in got:
        want = b.planes.get(r, port[r])  # the closed form where there is one, else the port
        assert bits64(got[r].c) == bits64(want.c) and bits64(got[r].n) == bits64(want.n), (fam, r, got[r], want)
    assert (set(b.planes) == set(got)) == (fam in EXACT)


# ---- table path ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_table_rows(ctx, fam):
    b = R.structure(fam)
    cutoff = R.TABLE_CUTOFF[fam]
    s = aa.Structure.from_records(b.rec)
    ring, atom = device_rows(ctx, s, b.top, cutoff)
    planes = device_planes(ctx, s, b.top)
    restated = R.ring_rows(b.top, b.xyz, planes, cutoff)
    assert ring == restated, ("device only", describe(b, fam, ring - restated), "restatement only", describe(b, fam, restated - ring))
    o_ring, o_atom = oracle_rows(b.top, b.rec, cutoff)
    assert atom == o_atom, (sorted(atom - o_atom)[:5], sorted(o_atom - atom)[:5])
    out = R.outcomes(b, ring)
    excluded = set()
    if fam in EXACT:
        assert ring == o_ring, ("device only", describe(b, fam, ring - o_ring), "oracle only", describe(b, fam, o_ring - ring))
    elif fam == "d":
        # fitted planes: the oracle's fit and the device's may differ in the last bits, and the device may differ from the oracle exactly at the
        # points where the restatement itself answers differently on the two sets of planes -- computed here, never listed by hand
        orc = ob.Structure.from_atoms(synth.records_to_oracle(b.rec, flat=False), flat=False)
        res = {k: r for r, k in enumerate(b.top.res_key)}
        o_planes = {res[(bytes(pl["chain"]), int(pl["resi"]))]: R.Plane(tuple(pl["c"].tolist()), tuple(pl["n"].tolist())) for pl in orc.planes("ring")}
        on_oracle = R.outcomes(b, R.ring_rows(b.top, b.xyz, o_planes, cutoff))
        excluded = {p for p in range(len(b.motifs)) if on_oracle[p] != out[p]}
        ent_res = [r for r, _ in b.top.rings]
        keep = lambda rows: {x for x in rows if ent_res[x[0] - b.top.n] not in excluded}
        assert keep(ring) == keep(o_ring)
        print(f"family d: {len(excluded)} of {len(b.motifs)} points excluded (restatement differs between the oracle's planes and the device's)")
    # the device run shows both outcomes of every sweep (the CPU file asserts the same of the oracle's rows)
    for si, sw in enumerate(R.sweeps(fam)):
        mine = [out[p] for p, (i, _, _) in enumerate(b.motifs) if i == si and p not in excluded]
        assert not sw.both or len(set(mine)) >= 2, (sw.label, mine)
        if fam in ("f3", "f4"):
            assert all(m == ((0, R.CATION_PI),) for m in mine), (sw.label, mine)


# ---- frame path ------------------------------------------------------------------------------------------------------------------------------
def expected_timeline(built, fr, cutoff: float) -> dict:
    F = len(built)
    out = {}
    for f, b in enumerate(built):
        planes = {**R.port_planes(b.top, fr[f]), **b.planes}  # the closed form where there is one, else the port (== the device's: test_planes)
        for frm, to, code, dbits in R.ring_rows(b.top, fr[f], planes, cutoff):
            e = out.setdefault((frm, to, code), ([False] * F, []))
            e[0][f] = True
            e[1].append(float(np.uint32(dbits).view(np.float32)))
    return {k: (tuple(p), min(d), max(d)) for k, (p, d) in out.items()}


def device_timeline(ctx, s, fr, cutoff: float, n: int) -> dict:
    t = ctx.contact_timelines(s, fr, "/", 0.1, cutoff, rings=True)
    F = fr.shape[0]
    present = aa.unpack_timeline(t["timeline_words"], F) if len(t["n_frames"]) else np.zeros((0, F), bool)
    out = {}
    for k in np.flatnonzero(t["from_ring"] >= 0):
        to = int(t["to_atom"][k]) if t["to_ring"][k] < 0 else n + int(t["to_ring"][k])
        key = (n + int(t["from_ring"][k]), to, int(t["interaction"][k]))
        assert key not in out
        assert int(t["n_frames"][k]) == int(present[k].sum())
        out[key] = (tuple(present[k].tolist()), float(t["min_distance"][k]), float(t["max_distance"][k]))
    return out


def frame_sweeps(fam):
    return [(fam, si) for si in range(len(R.sweeps(fam)))]


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_frame_rows(ctx, fam):
    """Every sweep of the family as frames of a one-motif topology: one pass, then two."""
    cutoff = R.TABLE_CUTOFF[fam]
    for si, sw in enumerate(R.sweeps(fam)):
        built, fr = R.frames(fam, si)
        want = expected_timeline(built, fr, cutoff)
        s = aa.Structure.from_records(built[0].rec)
        n, F = built[0].top.n, fr.shape[0]
        got = device_timeline(ctx, s, fr, cutoff, n)
        assert got == want, (sw.label, got, want)
        if sw.both:
            assert len({tuple(sorted(k for k, v in got.items() if v[0][f])) for f in range(F)}) >= 2, sw.label
        if F > 1:
            per = -(-F // 2)
            aa.debug_set("freq_chunk_atoms", per * n)
            assert device_timeline(ctx, s, fr, cutoff, n) == want, (sw.label, "two passes")
            aa.debug_set("freq_chunk_atoms", 0)


@pytest.mark.parametrize("fam", ("a", "b", "c", "d"))
def test_frame_rows_at_the_residue_level(ctx, fam):
    """Level 1: a ring row of residues (chain-A residue, partner residue, code) exists in a frame exactly when the restatement has an entity row there."""
    cutoff = R.TABLE_CUTOFF[fam]
    for si, sw in enumerate(R.sweeps(fam)):
        built, fr = R.frames(fam, si)
        top = built[0].top
        ent_res = [r for r, _ in top.rings]
        want = {}
        for (frm, to, code), (p, _, _) in expected_timeline(built, fr, cutoff).items():
            key = (ent_res[frm - top.n], top.res_of[to] if to < top.n else ent_res[to - top.n], code)
            want[key] = tuple(a or b for a, b in zip(want.get(key, (False,) * len(p)), p))
        s = aa.Structure.from_records(built[0].rec)
        t = ctx.contact_timelines(s, fr, "/", 0.1, cutoff, rings=True, level="residue")
        present = aa.unpack_timeline(t["timeline_words"], fr.shape[0]) if len(t["n_frames"]) else np.zeros((0, fr.shape[0]), bool)
        got = {(int(t["from_residue"][k]), int(t["to_residue"][k]), int(t["interaction"][k])): tuple(present[k].tolist())
               for k in range(len(t["n_frames"])) if int(t["interaction"][k]) in RING_CODES}
        assert got == want, (sw.label, got, want)
