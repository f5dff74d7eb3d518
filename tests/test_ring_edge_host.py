"""The ring-edge cases of tests/ring_edge_rules.py on the CPU: the restatement is held to the oracle before the device is held to the restatement.

  * the restatement on the oracle's planes gives the oracle's ring rows -- entities, code, distance -- on every family, as one structure per
    family and as the frames of every sweep
  * every sweep shows both outcomes; the search-edge motifs show a row at the cutoff and none beyond it
  * on the exact-plane families the oracle's planes and the ported fit ARE the closed form, bit for bit
  * the ported fit and the oracle's fit are each within a few eps of a 50-digit eigenvector (mpmath)
  * the quotients the hunts aim at are the doubles on which the host's acos flips the comparisons, and the hunts reach every one of them
"""
from __future__ import annotations

import math
import re

import numpy as np
import pytest

import oracle_binding as ob
import ring_edge_rules as R
import synth

EXACT = ("a", "b", "c", "f3", "f4")
RING_CODES = set(range(11, 18))


def oracle_of(rec):
    return ob.Structure.from_atoms(synth.records_to_oracle(rec, flat=False), flat=False)


def oracle_planes(top: R.Topology, orc) -> dict:
    res = {k: r for r, k in enumerate(top.res_key)}
    out = {}
    for pl in orc.planes("ring"):
        out[res[(bytes(pl["chain"]), int(pl["resi"]))]] = R.Plane(tuple(float(v) for v in pl["c"]), tuple(float(v) for v in pl["n"]))
    return out


def oracle_ring_rows(top: R.Topology, rows) -> set:
    ent = {(top.res_key[r][0], top.res_key[r][1], alt): e for e, (r, alt) in enumerate(top.rings)}
    out = set()
    for r in rows:
        if int(r["interaction"]) not in RING_CODES:
            continue
        f, t = r["from"], r["to"]
        frm = top.n + ent[(bytes(f["chain"]), int(f["resi"]), bytes(f["altloc"]))]
        to = int(r["to_atom"]) if int(r["to_atom"]) >= 0 else top.n + ent[(bytes(t["chain"]), int(t["resi"]), bytes(t["altloc"]))]
        out.add((frm, to, int(r["interaction"]), int(np.float32(r["distance"]).view(np.uint32))))
    return out


@pytest.fixture(scope="module")
def oracle_runs():
    out = {}
    for fam in R.FAMILIES:
        b = R.structure(fam)
        orc = oracle_of(b.rec)
        out[fam] = (oracle_planes(b.top, orc), oracle_ring_rows(b.top, orc.get_contacts("/", 0.1, R.TABLE_CUTOFF[fam])))
    return out


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_sizes(fam):
    b = R.structure(fam)
    assert b.top.n < 4000 and len(b.top.rings) < 1088


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_restatement_on_the_oracles_planes_is_the_oracle(oracle_runs, fam):
    b = R.structure(fam)
    planes, rows = oracle_runs[fam]
    assert set(planes) == {r for r, ra in enumerate(b.top.ring_atoms) if ra}
    assert R.ring_rows(b.top, b.xyz, planes, R.TABLE_CUTOFF[fam]) == rows
    assert len(rows) > 0


@pytest.mark.parametrize("fam", EXACT)
def test_exact_planes_are_the_closed_form_bit_for_bit(oracle_runs, fam):
    b = R.structure(fam)
    planes, rows = oracle_runs[fam]
    assert set(b.planes) == set(planes)
    port = R.port_planes(b.top, b.xyz)
    for r, want in b.planes.items():
        assert planes[r] == want, (r, planes[r], want)   # (tuples of floats: == is bit equality up to the sign of zero, asserted next)
        assert port[r] == want, (r, port[r], want)
        assert all(math.copysign(1.0, v) == 1.0 for v in planes[r].n + port[r].n)
    assert R.ring_rows(b.top, b.xyz, b.planes, R.TABLE_CUTOFF[fam]) == rows


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_every_sweep_shows_both_outcomes(oracle_runs, fam):
    b = R.structure(fam)
    out = R.outcomes(b, oracle_runs[fam][1])
    sw = R.sweeps(fam)
    for si, s in enumerate(sw):
        mine = [out[p] for p, (i, _, _) in enumerate(b.motifs) if i == si]
        assert len(mine) == s.n_points
        if s.both:
            assert len(set(mine)) >= 2, (s.label, mine)
        if fam in ("f3", "f4"):  # a row to the cation at the cutoff, none to the one beyond, at every slide position and in both corners
            assert all(m == ((0, R.CATION_PI),) for m in mine), (s.label, mine)
        if fam == "e" and "on axis" not in s.label and "collinear" not in s.label:
            assert all(len(m) >= 1 and all(c == R.CATION_PI for _, c in m) for m in mine), (s.label, mine)
    if fam == "e":  # the cations on the axes of fitted rings land on both sides of q = 1
        on_axis = [out[p] for p, (i, _, _) in enumerate(b.motifs) if "on axis" in sw[i].label]
        assert () in on_axis and ((0, R.CATION_PI),) in on_axis, on_axis
    if fam == "b":
        special = {s.label: out[p] for p, (i, _, _) in enumerate(b.motifs) for s in [sw[i]] if not s.both}
        assert special == {"concentric perpendicular": ((0, R.TSTACK),), "cation on the centre": (), "theta exactly 90": ((0, R.INPLANE),)}


def test_search_edge_structures_reach_the_box_corners():
    for fam in ("f3", "f4"):
        b = R.structure(fam)
        xyz = b.xyz
        first, last = b.top.res_atoms[0] + sum((b.top.res_atoms[r] for r in b.b_res[0]), []), b.top.res_atoms[len(b.motifs) - 1] + sum(
            (b.top.res_atoms[r] for r in b.b_res[-1]), [])
        for k in range(3):
            assert int(np.argmin(xyz[:, k])) in first and int(np.argmax(xyz[:, k])) in last


@pytest.mark.parametrize("fam", ("a", "b", "c", "f3"))
def test_frames_of_every_sweep(fam):
    """The frame form: one motif at the origin, a frame per sweep point.  Restatement on the closed form == oracle, frame by frame."""
    for si, s in enumerate(R.sweeps(fam)):
        built, fr = R.frames(fam, si)
        seen = []
        for f, b in enumerate(built):
            orc = oracle_of(b.rec)
            want = oracle_ring_rows(b.top, orc.get_contacts("/", 0.1, R.TABLE_CUTOFF[fam]))
            assert oracle_planes(b.top, orc) == b.planes, (s.label, f)
            assert R.ring_rows(b.top, fr[f], b.planes, R.TABLE_CUTOFF[fam]) == want, (s.label, f)
            seen.append(tuple(sorted((x[0], x[1], x[2]) for x in want)))
        if s.both:
            assert len(set(seen)) >= 2, (s.label, seen)


def test_hunt_targets_are_the_flips_of_the_hosts_acos():
    for T in (30.0, 60.0):
        for sign in (1, -1):
            qs = R.hunt_targets(T, sign)
            ang = [R.angle_of_q(q) for q in qs]
            assert 2 <= len(qs) <= 3 and all(R.step(a, 1) == b for a, b in zip(qs, qs[1:]))
            assert min(ang) <= T <= max(ang) and (min(ang) < T or max(ang) > T)
            # one step of q moves the angle by ulp(q) / sin T radians: 3.6 ulps of 30 degrees, 0.6 ulps of 60
            assert all(abs(a - T) <= 8 * math.ulp(T) for a in ang), (T, sign, ang)
            inside = [a <= T for a in ang]
            assert True in inside and False in inside
            print(f"T={T} sign={sign}: q = {[q.hex() for q in qs]}, angle - T in ulps = {[round((a - T) / math.ulp(T)) for a in ang]}")


def test_no_quotient_gives_exactly_30_or_60():
    """fold_deg(acos q) steps over 30.0 and over 60.0 on both sides of the ring: `<= T` and `< T` are the same predicate of q.  So a `<=`
    turned into `<` at an angle threshold is no wrong answer, and the device's `<` and `<=` bounds coincide."""
    for T in (30.0, 60.0):
        for sign in (1, -1):
            qs = R.hunt_targets(T, sign)
            assert len(qs) == 2 and all(R.angle_of_q(q) != T for q in qs)


def test_cosine_bounds_of_the_ring_rules():
    """table_dev.hip decides the ring angle rules on q against eight constants: each must be the extreme q that the C library's acos and
    fold_deg still put on the stated side of its threshold, and the next double must be on the other side."""
    src = (synth.DATA.parent.parent / "arpeggia_amd" / "csrc" / "table_dev.hip").read_text()
    const = {m.group(1): float.fromhex(m.group(2)) for m in re.finditer(r"constexpr double (kCos\w+) = ([-0-9a-fx.p]+);", src)}
    ang = R.angle_of_q
    rules = {"Le30": lambda a: a <= 30.0, "Ge30": lambda a: a >= 30.0, "Le60": lambda a: a <= 60.0, "Lt60": lambda a: a < 60.0}
    assert set(const) == {f"kCos{r}{s}" for r in rules for s in ("Pos", "Neg")}
    for name, q in const.items():
        rule, pos = rules[name[4:8]], name.endswith("Pos")
        assert (q > 0.0) == pos and rule(ang(q)), (name, q)
        # the angle falls with q for q > 0 and rises with q for q < 0: `<=` / `<` hold from the bound outwards (towards +-1), `>=` inwards
        outwards = 1 if pos else -1
        beyond = R.step(q, -outwards if name[4:6] in ("Le", "Lt") else outwards)
        assert not rule(ang(beyond)), (name, q, beyond)
        # and the bound is found again by bisection over the doubles
        q0 = (1 if pos else -1) * math.cos(math.radians(float(name[6:8])))
        b = R.find_flip(lambda x: rule(ang(x)), q0 - 1e-9, q0 + 1e-9)
        assert q in (b, R.step(b, -1)), (name, q, b)
    # the ends: every q of [-1, 1] is <= 90, +-1 are inside 30, 0 is outside 60, and NaN or |q| > 1 has no angle
    assert ang(1.0) == 0.0 and ang(-1.0) <= 30.0 and ang(0.0) == 90.0 and ang(-0.0) == 90.0
    assert all(a != a for a in (ang(R.step(1.0, 1)), ang(R.step(-1.0, -1)), ang(math.nan)))
    assert max(ang(R.step(0.0, 1)), ang(R.step(0.0, -1)), ang(1e-17), ang(-1e-17)) <= 90.0


def test_hunts_reach_every_target():
    """The yield of the seeded searches: every hunt sweep has a geometry for each of its targets, on the lattice and at the origin."""
    b = R.structure("c")
    n = 0
    for p, (si, j, m) in enumerate(b.motifs):
        s = R.sweeps("c")[si]
        T, sign = (30.0 if " 30 " in s.label else 60.0), (1 if s.label.endswith("+") else -1)
        target = R.hunt_targets(T, sign)[j]
        q = m.partners[0][0] if len(m.partners[0]) == 1 else m.b_planes[0].c
        assert R.point_q(m.a_plane, q) == target, (s.label, j)
        n += 1
    assert n == sum(s.n_points for s in R.sweeps("c")) >= 28
    exact = [s.label for s in R.sweeps("c") for j in range(s.n_points)
             if R.angle_of_q(R.hunt_targets(30.0 if " 30 " in s.label else 60.0, 1 if s.label.endswith("+") else -1)[j]) in (30.0, 60.0)]
    print("hunt geometries with an angle of exactly T:", exact)


def _mp_normal(pts):
    import mpmath as mp

    mp.mp.dps = 50
    P = [[mp.mpf(float(v)) for v in p] for p in pts]
    n = len(P)
    c = [sum(p[k] for p in P) / n for k in range(3)]
    A = mp.matrix(3, 3)
    for p in P:
        d = [p[k] - c[k] for k in range(3)]
        for i in range(3):
            for j in range(3):
                A[i, j] += d[i] * d[j]
    E, Q = mp.eigsy(A)
    k = min(range(3), key=lambda i: E[i])
    return [Q[i, k] for i in range(3)]


def _angle_to(ref, n):
    import mpmath as mp

    v = [mp.mpf(x) for x in n]
    cr = [ref[1] * v[2] - ref[2] * v[1], ref[2] * v[0] - ref[0] * v[2], ref[0] * v[1] - ref[1] * v[0]]
    s = mp.sqrt(sum(x * x for x in cr)) / (mp.sqrt(sum(x * x for x in ref)) * mp.sqrt(sum(x * x for x in v)))
    return float(mp.asin(min(s, mp.mpf(1))))


def test_fit_errors_against_a_50_digit_eigenvector(oracle_runs):
    """Largest angle (radians) between the fitted normal and the 50-digit one, per family, for the ported device fit and for the oracle's.
    Both Jacobi variants are backward stable and the in-plane / out-of-plane eigenvalue gap of a ring is of the order of the matrix norm, so a
    few eps is the expectation; 64 eps is asserted."""
    worst = {}
    for fam in ("a", "b", "d", "e"):
        b = R.structure(fam)
        port, orc = R.port_planes(b.top, b.xyz), oracle_runs[fam][0]
        ep = eo = 0.0
        for r, ra in enumerate(b.top.ring_atoms):
            if not ra or (r < len(b.motifs) and "collinear" in R.sweeps(fam)[b.motifs[r][0]].label):
                continue  # (a line has no plane: the 50-digit eigenvector of a tied spectrum is any vector across it)
            ref = _mp_normal(b.xyz[ra])
            ep, eo = max(ep, _angle_to(ref, port[r].n)), max(eo, _angle_to(ref, orc[r].n))
        worst[fam] = (ep, eo)
        print(f"family {fam}: largest normal error  port {ep:.3e} rad  oracle {eo:.3e} rad")
    assert worst["a"] == (0.0, 0.0) and worst["b"] == (0.0, 0.0)
    assert max(worst["d"] + worst["e"]) <= 64 * 2.0 ** -52
