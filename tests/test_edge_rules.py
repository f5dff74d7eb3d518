"""The contact rules at their decision boundaries, on the CPU: the plain restatement (tests/edge_rules.py) against the oracle on the edge
motif sets and on real inputs, the host's squared-distance bounds against their definition, and the three radius tables against each other.
The same sets go through the HIP path in test_edge_rules_gpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

import edge_rules as E
import oracle_binding as ob
import synth


def _oracle_pairs(es, groups, c, cutoff):
    orc = ob.Structure.from_atoms(synth.records_to_oracle(es.records(), flat=False), flat=False)
    w = orc.atomic_contacts(groups, c, cutoff)
    return {(int(i), int(j)): (int(k), float(d)) for i, j, k, d in zip(w["i"], w["j"], w["kind"], w["dist"])}


def _assert_same(restated, oracle, what):
    missing = sorted(set(restated) - set(oracle))[:3]
    extra = sorted(set(oracle) - set(restated))[:3]
    assert not missing and not extra, f"{what}: pair sets differ (restatement only {missing}, oracle only {extra})"
    bad = [p for p in restated if restated[p][0] != oracle[p][0]]
    assert not bad, f"{what}: {len(bad)} kind mismatches, first {bad[0]}: restatement {restated[bad[0]][0]:#x} oracle {oracle[bad[0]][0]:#x}"
    bad = [p for p in restated if restated[p][1] != oracle[p][1]]
    assert not bad, f"{what}: {len(bad)} distance mismatches, first {bad[0]}"


# ---------------------------------------------------------------------------------------------- (a) restatement == oracle on the edge sets
@pytest.mark.parametrize("place", E.PLACES)
@pytest.mark.parametrize("family", E.FAMILIES)
@pytest.mark.parametrize("vdw_comp", E.VDW_COMPS)
def test_restatement_matches_oracle_on_edge_sets(vdw_comp, family, place):
    es = E.gen_edges(family, vdw_comp, place)
    # the radii family is 2 x 10^4 atoms: every cutoff near the origin, the far copies at the cutoffs that reach every radius bound
    cutoffs = E.CUTOFFS if (family == "rules" or place == "origin") else (6.5, 12.0)
    for cutoff in cutoffs:
        what = f"{family} {place} c={vdw_comp} d={cutoff}"
        r = E.contacts(es.atoms, "/", vdw_comp, cutoff)
        assert not E.vacuous(es, r, cutoff), f"{what}: sweeps with one outcome only: {E.vacuous(es, r, cutoff)[:5]}"
        _assert_same(r, _oracle_pairs(es, "/", vdw_comp, cutoff), what)


def test_edge_sets_cover_what_they_claim():
    """The generator's own promises: the radii set stays on the small-input route; the 90-degree sweeps hold an angle of exactly 90.0; the
    f32 sweeps hold an exact tie and cross the 2048-ulp window on both sides; the far copies span +-9999 A."""
    radii = E.gen_edges("radii", 0.1, "far+")
    assert len(radii.atoms) < 20480
    xs = np.array([a.xyz for a in radii.atoms])
    assert xs.max() >= 9950.0 and xs.min() <= -9990.0
    rules = E.gen_edges("rules", 0.1, "origin")
    exact90 = 0
    for sw in rules.sweeps:
        if sw.label.startswith("angle 90"):
            for x, y in sw.pairs:
                h = next(k for k in E.residue_index(rules.atoms)[rules.atoms[x].res] if rules.atoms[k].elem == "H")
                exact90 += E.angle(rules.atoms[x].xyz, rules.atoms[h].xyz, rules.atoms[y].xyz) == 90.0
    assert exact90 >= 2
    r = E.contacts(rules.atoms, "/", 0.1, 6.5)
    for sw in (s for s in rules.sweeps if s.kind == "f32"):
        offs = [(r[p][1] - sw.bound) / math.ulp(sw.bound) for p in sw.pairs]
        assert 0.0 in offs and min(offs) < -2048 and max(offs) > 2048 and any(0 < abs(o) <= 3 for o in offs), sw.label


# ---------------------------------------------------------------------------------------------- (b) restatement == oracle on real inputs
def _restated_kinds(orc, pairs, c):
    at = orc.atoms
    atoms = [E.Atom((float(a["x"]), float(a["y"]), float(a["z"])), a["name"].decode(), a["resn"].decode(), a["res_resn"].decode(),
                    a["elem"].decode(), a["chain"].decode(), int(a["model_idx"]), int(a["res_idx"]), int(a["res_ord"])) for a in at]
    res_atoms = E.residue_index(atoms)
    ok = lambda k: atoms[k].resn in E.EDGE_RESIDUES and atoms[k].res_resn in E.EDGE_RESIDUES
    sel = [n for n in range(len(pairs)) if ok(int(pairs["i"][n])) and ok(int(pairs["j"][n]))]
    got = np.array([E.classify(atoms, res_atoms, int(pairs["i"][n]), int(pairs["j"][n]), c) for n in sel], dtype=np.uint32)
    return np.array(sel, dtype=np.int64), got


@pytest.mark.parametrize("name", ["1ubq", "6bft", "stress"])
def test_restatement_matches_oracle_on_real_inputs(name):
    if name == "stress":
        rec = synth.gen_stress(n_res=400, seed=7)  # hydrogens on the donors: the angle branches
        orc = ob.Structure.from_atoms(synth.records_to_oracle(rec, flat=False), flat=False)
    else:
        orc = ob.Structure.load(str(synth.DATA / f"{name}.pdb"))
    for c in (0.1, -0.6, 1.0):
        want = orc.atomic_contacts("/", c, 6.5)
        sel, got = _restated_kinds(orc, want, c)
        assert len(sel) > 300, name
        bad = np.flatnonzero(got != want["kind"][sel])
        assert len(bad) == 0, f"{name} c={c}: {len(bad)} kind mismatches, first pair {want[sel[bad[0]]]} restatement {got[bad[0]]:#x}"
        seen = np.bitwise_or.reduce(got)
        for rule in ("VanDerWaalsContact", "PolarContact", "HydrophobicContact") if c == 0.1 else ():
            assert seen & E.BIT[rule], f"{name}: no {rule} among the compared pairs"
        if name == "stress" and c == 0.1:
            for rule in ("StericClash", "CovalentBond", "HydrogenBond", "WeakHydrogenBond", "IonicBond", "SaltBridge", "IonicRepulsion", "Disulfide"):
                assert seen & E.BIT[rule], f"stress: no {rule} among the compared pairs"


# ---------------------------------------------------------------------------------------------- (c) the host's bounds
def _bound_fns():
    from arpeggia_amd import _lib

    lib = _lib.lib
    fns = []
    for sym in ("_ZN3arp8bound_ltEd", "_ZN3arp8bound_leEd"):  # arp::bound_lt / arp::bound_le (engine.cpp; the library exports default visibility)
        f = getattr(lib, sym)
        f.restype, f.argtypes = C.c_double, [C.c_double]
        fns.append(f)
    return fns


def _thresholds():
    ts = {0.0, 3.5, 4.0, 4.5, *E.CUTOFFS}
    for c in E.VDW_COMPS:
        for ea, (ca, va) in E.RADII.items():
            ts.add(E.RADII["H"][1] + va + c)
            for eb, (cb, vb) in E.RADII.items():
                ts.update((ca + cb - c, ca + cb + c, va + vb + c))
    return sorted(ts)


def test_squared_distance_bounds_meet_their_definition():
    """bound_lt(T) = min{s >= 0 : sqrt(s) >= T} and bound_le(T) = min{s >= 0 : sqrt(s) > T} (arp_internal.h DevParams), so that
    sqrt(s) < T <=> s < bound_lt(T) and sqrt(s) <= T <=> s < bound_le(T) for every s >= 0: checked with the correctly rounded math.sqrt on
    every threshold the default radii make with the compensation factors of the suite, and on the awkward ones."""
    lt, le = _bound_fns()
    ts = _thresholds()
    assert len(ts) > 500
    big = 1.5e154  # T^2 overflows
    for T in ts + [-1.0, -0.0, 5e-324, 2.2250738585072014e-308 / 3, 1e-160, big, 1e300, math.inf, math.nan]:
        for f, cmp in ((lt, lambda d, T: d < T), (le, lambda d, T: d <= T)):
            b = f(T)
            if math.isnan(T) or T < 0.0 or (T == 0.0 and f is lt):
                assert b == 0.0, (f, T, b)  # nothing is below (or at) such a T
                continue
            if math.isinf(b):
                assert not cmp(math.inf, T) or math.isinf(T), (T, b)
                assert cmp(math.sqrt(1.7976931348623157e308), T), (T, b)  # every finite s decides "inside"
                continue
            assert not cmp(math.sqrt(b), T), (T, b)                       # b itself is outside
            if b > 0.0:
                assert cmp(math.sqrt(E.step(b, -1)), T), (T, b)           # and the double below it inside
            for k in range(-3, 4):                                       # the equivalence around the bound
                s = E.step(b, k)
                if s >= 0.0:
                    assert cmp(math.sqrt(s), T) == (s < b), (T, b, k)


# ---------------------------------------------------------------------------------------------- (d) the radius tables
def test_three_radius_tables_agree():
    import arpeggia_amd as aa
    from arpeggia_amd import _lib

    p = aa.default_params()
    for sym, (cov, vdw) in E.RADII.items():
        k = _lib.lib.arp_element_class(sym.encode())
        assert k >= 0, sym
        assert (p.cov_radius[k], p.vdw_radius[k]) == (cov, vdw), f"{sym}: product {p.cov_radius[k], p.vdw_radius[k]} restatement {cov, vdw}"
        oc, ov = C.c_double(), C.c_double()
        assert ob.lib().orc_radii(sym.encode(), C.byref(oc), C.byref(ov)), sym
        assert (oc.value, ov.value) == (cov, vdw), f"{sym}: oracle {oc.value, ov.value} restatement {cov, vdw}"
    assert p.h_vdw_radius == E.RADII["H"][1]
    assert sorted(_lib.lib.arp_element_class(s.encode()) for s in E.RADII) == list(range(16))


# ---------------------------------------------------------------------------------------------- the device's angle thresholds
def test_cosine_bounds_of_the_angle_rules():
    """kernels.hip decides the angle rules on q = dot / (|u| |v|) against four constants: each must be the extreme q that the C library's
    acos (what the reference calls) still puts on the inside of its threshold, and the next double must be outside."""
    import re

    src = (synth.DATA.parent.parent / "arpeggia_amd" / "csrc" / "kernels.hip").read_text()
    const = {m.group(1): float.fromhex(m.group(2)) for m in re.finditer(r"constexpr double (kCos\w+) = ([-0-9a-fx.p]+);", src)}
    ang = lambda q: E._acos(q) * E.RAD2DEG
    for name, T, ge in (("kCosHbond", 90.0, True), ("kCosWeakHbond", 130.0, True), ("kCosDisulfideLo", 60.0, True), ("kCosDisulfideHi", 120.0, False)):
        q = const[name]
        if ge:  # largest q with angle >= T
            assert ang(q) >= T and ang(E.step(q, 1)) < T, (name, q)
        else:   # smallest q with angle <= T
            assert ang(q) <= T and ang(E.step(q, -1)) > T, (name, q)
    assert E.angle((1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)) == 90.0 and const["kCosHbond"] > 0.0  # (0 is inside: >= 90)
