"""The HIP path at the contact rules' decision boundaries: the edge motif sets of tests/edge_rules.py through every emitter route, against
the plain restatement (kind bits, pair set, and the f32 distance, which must be float32(math.sqrt(s)) bit for bit).  The CPU half
(test_edge_rules.py) holds the restatement to the oracle on the same sets."""
import math
import os

import numpy as np
import pytest

import arpeggia_amd as aa
import edge_rules as E
import synth

pytestmark = pytest.mark.gpu

SMALL_ROUTE, STAGE_ROUTE = 20480, 131072  # emit_plan.h: kDirectTasks (320 tasks of 64), kStageTasks (2048 tasks)


@pytest.fixture(scope="module")
def ctx():
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


_restated = {}


def restated(es, groups="/", cutoff=6.5):
    key = (es.family, es.vdw_comp, es.place, groups, cutoff)
    if key not in _restated:
        _restated[key] = E.contacts(es.atoms, groups, es.vdw_comp, cutoff)
    return _restated[key]


def check(got, want, what):
    """Product pairs against the restatement's {(i, j): (kind, d, s)}; returns the number of pairs compared."""
    g = {(int(i), int(j)): (int(k), d) for i, j, k, d in zip(got["i"], got["j"], got["kind"], got["dist"])}
    assert len(g) == len(got), f"{what}: duplicate pairs"
    only_g, only_w = sorted(set(g) - set(want))[:3], sorted(set(want) - set(g))[:3]
    assert not only_g and not only_w, f"{what}: pair sets differ ({len(set(g) ^ set(want))}): product only {only_g}, restatement only {only_w}"
    bad = [p for p in want if g[p][0] != want[p][0]]
    assert not bad, f"{what}: {len(bad)} kind mismatches, first {bad[0]} d={want[bad[0]][1]!r}: product {g[bad[0]][0]:#x} restatement {want[bad[0]][0]:#x}"
    bad = [p for p in want if g[p][1] != np.float32(math.sqrt(want[p][2]))]
    assert not bad, f"{what}: {len(bad)} f32 distances differ, first {bad[0]}: product {g[bad[0]][1]!r} float32(sqrt(s)) {np.float32(want[bad[0]][1])!r}"
    return len(want)


def _only(want):
    return {p: v for p, v in want.items() if v[0] != 0}


def _pad(rec, n_total, x0=600.0):
    """Inert carbons (one residue each, chain P) 14 A apart on a lattice beyond the motifs, up to n_total atoms: no pair among them."""
    n = n_total - len(rec["x"])
    side = math.ceil(n ** (1.0 / 3.0))
    k = np.arange(n)
    xyz = np.stack([x0 + 14.0 * (k // (side * side)), 14.0 * ((k // side) % side), 14.0 * (k % side)], 1)
    pad = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "occupancy": np.ones(n), "serial": np.arange(len(rec["x"]) + 1, n_total + 1, dtype=np.int32),
           "resi": (k + 1).astype(np.int32), "model_serial": np.zeros(n, dtype=np.int32), "name": np.full(n, b"CQ", dtype="S8"),
           "resn": np.full(n, b"GLY", dtype="S8"), "chain": np.full(n, b"P", dtype="S8"), "altloc": np.zeros(n, dtype="S4"),
           "icode": np.zeros(n, dtype="S4"), "element": np.full(n, b"C", dtype="S4")}
    return {c: np.concatenate([rec[c], pad[c]]) for c in rec}


def _report(route, n):
    print(f"edge pairs [{route}]: {n}")


# ---------------------------------------------------------------------------------------------- the small-input route, every parameter
@pytest.mark.parametrize("place", E.PLACES)
@pytest.mark.parametrize("family", E.FAMILIES)
@pytest.mark.parametrize("vdw_comp", E.VDW_COMPS)
def test_edge_sets_small_route(ctx, vdw_comp, family, place):
    es = E.gen_edges(family, vdw_comp, place)
    prod = aa.Structure.from_records(es.records())
    assert prod.n_atoms == len(es.atoms) < SMALL_ROUTE  # the hole-free sequence of small inputs (4-wave k_emit)
    soa = prod.soa("/")
    cutoffs = E.CUTOFFS if vdw_comp == 0.1 or family == "rules" else (6.5,)
    n = 0
    for cutoff in cutoffs:
        want = restated(es, "/", cutoff)
        what = f"{family} {place} c={vdw_comp} d={cutoff}"
        n += check(ctx.atomic_contacts(soa, aa.default_params(vdw_comp, cutoff)), want, what)
        n += check(ctx.atomic_contacts(soa, aa.default_params(vdw_comp, cutoff, deterministic=True)), want, what + " ordered")
        n += check(ctx.atomic_contacts(soa, aa.default_params(vdw_comp, cutoff, contacts_only=True)), _only(want), what + " contacts only")
        n += check(ctx.atomic_contacts(soa, aa.default_params(vdw_comp, cutoff, deterministic=True, contacts_only=True)), _only(want), what + " ordered, contacts only")
    _report(f"small {family} {place} c={vdw_comp}", n)


# ---------------------------------------------------------------------------------------------- the larger routes: padded sets, strips
@pytest.mark.parametrize("vdw_comp", [0.1, -0.6, 1.0])
@pytest.mark.parametrize("n_total", [40000, 140000])
def test_edge_sets_padded_through_the_larger_kernels(ctx, n_total, vdw_comp):
    """The edge sets padded with inert far-apart atoms past 20 480 atoms (the 12-wave k_emit, staged once the context knows the input defers
    nothing) and past 131 072 (plain k_emit with chunks and the fix-up), with and without the residue-rule kernels, twice each (the memos)."""
    for family in E.FAMILIES:
        es = E.gen_edges(family, vdw_comp, "origin")
        prod = aa.Structure.from_records(_pad(es.records(), n_total))
        assert prod.n_atoms == n_total and n_total > (SMALL_ROUTE if n_total < STAGE_ROUTE else STAGE_ROUTE)
        soa = prod.soa("/")
        want = restated(es)
        n = 0
        for runs in (True, False):
            for k in range(2):
                n += check(ctx.atomic_contacts(soa, aa.default_params(vdw_comp, 6.5, residue_runs=runs)), want, f"{family} {n_total} runs={runs} call {k}")
            n += check(ctx.atomic_contacts(soa, aa.default_params(vdw_comp, 6.5, contacts_only=True, residue_runs=runs)), _only(want), f"{family} {n_total} only")
        n += check(ctx.atomic_contacts(soa, aa.default_params(vdw_comp, 6.5, deterministic=True)), want, f"{family} {n_total} ordered")
        _report(f"padded {n_total} {family} c={vdw_comp}", n)


@pytest.mark.parametrize("rows", [2, 8])
def test_edge_sets_on_forced_strips(rows):
    aa.debug_set("strip_rows", rows)  # (read when a context builds its parameter block: the fresh context below)
    try:
        ctx = aa.Context(0)
        for family in E.FAMILIES:
            es = E.gen_edges(family, 0.1, "origin")
            want = restated(es)
            n = 0
            for n_total in (len(es.atoms), 40000):
                soa = aa.Structure.from_records(_pad(es.records(), n_total) if n_total > len(es.atoms) else es.records()).soa("/")
                for k in range(2):
                    n += check(ctx.atomic_contacts(soa), want, f"{family} {n_total} strips of {rows}, call {k}")
                n += check(ctx.atomic_contacts(soa, aa.default_params(deterministic=True)), want, f"{family} {n_total} strips of {rows}, ordered")
            _report(f"strips {rows} {family}", n)
    finally:
        aa.debug_set("strip_rows", int(os.environ.get("ARP_TEST_STRIP_ROWS", "0")))  # (conftest.py: the suite may be running on strips)


# ---------------------------------------------------------------------------------------------- chain groups, packed batches, the table
@pytest.mark.parametrize("groups", ["A/B", "B/A", "A/", "/A", "B,Z/A"])
def test_edge_sets_chain_groups(ctx, groups):
    """Every motif pair has one atom in chain A and one in chain B: "B/A" makes the other atom the ligand (the donor tried first, the
    dihedral's argument order), the one-sided forms take the complement."""
    n = 0
    for family in E.FAMILIES:
        for place in ("origin", "far-"):
            es = E.gen_edges(family, 0.25, place)
            soa = aa.Structure.from_records(es.records()).soa(groups)
            want = restated(es, groups)
            assert len(want) > 100
            for det in (False, True):
                n += check(ctx.atomic_contacts(soa, aa.default_params(0.25, 6.5, deterministic=det)), want, f"{family} {place} {groups} det={det}")
    _report(f"groups {groups}", n)


def test_edge_sets_in_one_packed_batch(ctx):
    sets = [E.gen_edges(f, 0.1, p) for f in E.FAMILIES for p in E.PLACES]
    soas = [aa.Structure.from_records(es.records()).soa("/") for es in sets]
    got = aa.atomic_contacts_batch([ctx], soas, aa.default_params(0.1, 6.5))
    assert len(got) == len(sets)
    n = sum(check(g, restated(es), f"batch member {es.family} {es.place}") for g, es in zip(got, sets))
    _report("packed batch", n)


def test_edge_set_table_rows(ctx):
    """get_contacts on an edge set (plus one far-away PHE: the table path wants a ring, complex.rs:480-482): one row per set bit of every
    restated pair, with the pair's f32 distance."""
    es = E.gen_edges("rules", 0.1, "origin")
    rec = es.records()
    ubq = synth.read_pdb_records(synth.DATA / "1ubq.pdb")
    phe = np.flatnonzero((ubq["resn"] == b"PHE") & (ubq["resi"] == 4))
    n0 = len(rec["x"])
    extra = {c: ubq[c][phe].copy() for c in rec}
    for c, v in (("x", -300.0), ("y", -300.0), ("z", -300.0)):
        extra[c] = extra[c] + v
    extra["chain"][:] = b"Y"
    extra["serial"] = np.arange(n0 + 1, n0 + 1 + len(phe), dtype=np.int32)
    table = ctx.get_contacts(aa.Structure.from_records({c: np.concatenate([rec[c], extra[c]]) for c in rec}), "/", 0.1, 6.5)
    want = []
    for (i, j), (kind, d, s) in restated(es).items():
        for b in range(len(E.INTERACTIONS)):
            if kind >> b & 1:
                want.append((b, float(np.float32(d)), min(i, j) + 1, max(i, j) + 1))
    fa, ta = table["from_atomi"].astype(np.int64), table["to_atomi"].astype(np.int64)
    got = [(int(k), float(d), int(min(a, b)), int(max(a, b))) for k, d, a, b in zip(table["interaction"], table["distance"], fa, ta)]
    assert sorted(got) == sorted(want)
    _report("table rows", len(want))
