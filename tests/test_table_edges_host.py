"""The built cases of tests/table_edge_cases.py on the CPU: the oracle's table of every case has the closed-form counts, its longest run of rows that
agree in the ten sort keys is the named length (and sits where the case places it), the key widths are the named ones -- so every case reaches the edge it
is named for by construction, before a device is involved (tests/test_table_edges_gpu.py)."""
import numpy as np
import pytest

import oracle_binding as ob
import table_edge_cases as tec

CASES = tec.all_cases()
CATION_PI = ob.INTERACTIONS.index("CationPi")
IONIC, VDW = ob.INTERACTIONS.index("IonicBond"), ob.INTERACTIONS.index("VanDerWaalsContact")


def ten_keys(rows):
    f, t = rows["from"], rows["to"]
    return list(zip(rows["model"].tolist(), f["chain"].tolist(), t["chain"].tolist(), f["resi"].tolist(), f["altloc"].tolist(), f["atomi"].tolist(), t["resi"].tolist(),
                    t["altloc"].tolist(), t["atomi"].tolist(), rows["interaction"].tolist()))


def runs(rows):
    """[(start, length)] of the maximal runs of consecutive rows with equal ten keys."""
    keys, out, lo = ten_keys(rows), [], 0
    for p in range(1, len(keys) + 1):
        if p == len(keys) or keys[p] != keys[lo]:
            out.append((lo, p - lo))
            lo = p
    return out


def test_the_motif_states():
    """One motif per distance: the rows the case arithmetic counts with."""
    for d, want in ((tec.D_TWO, [IONIC, VDW]), (tec.D_ONE, [IONIC]), (tec.D_NONE, [])):
        kw = {"two": 0, "one": 0, "none": 0}
        kw[{tec.D_TWO: "two", tec.D_ONE: "one", tec.D_NONE: "none"}[d]] = 1
        c = tec.compose("probe", **kw)
        o = ob.Structure.from_atoms(tec.synth.records_to_oracle(c.rec, flat=False), flat=False)
        rows = o.get_contacts("/", tec.VDW_COMP, tec.CUTOFF)
        assert sorted(rows["interaction"].tolist()) == sorted(want)
        pairs = o.atomic_contacts("/", tec.VDW_COMP, tec.CUTOFF)
        assert len(pairs) == 1 and abs(float(pairs["dist"][0]) - d) < 1e-12  # a candidate pair in every state
        # 0.05 A to either side is the same state: no rule threshold nearby
        for dd in (-0.05, 0.05):
            rec = {k: v.copy() for k, v in c.rec.items()}
            rec["x"][-1] += dd
            o2 = ob.Structure.from_atoms(tec.synth.records_to_oracle(rec, flat=False), flat=False)
            assert sorted(o2.get_contacts("/", tec.VDW_COMP, tec.CUTOFF)["interaction"].tolist()) == sorted(want), (d, dd)


@pytest.mark.parametrize("name", list(CASES))
def test_counts_runs_and_widths(name):
    c = CASES[name]
    for groups in c.groups:
        rows = tec.oracle_rows(name, groups)
        ring = int((rows["interaction"] == CATION_PI).sum())
        assert (len(rows), ring, len(rows) - ring) == (c.rows, c.ring_rows, c.atom_rows), groups
        rr = runs(rows)
        longest = max((n for _, n in rr), default=1)
        assert longest == c.tie_run, groups
        if c.run_start >= 0:
            assert [lo for lo, n in rr if n == c.tie_run] == [c.run_start], groups
    pairs = tec.oracle_structure(name).atomic_contacts("/", tec.VDW_COMP, tec.CUTOFF)
    assert int((pairs["kind"] != 0).sum()) == c.pairs
    # key widths, restated from the records: chains, and the entities of the largest chain -- distinct (resi, altloc, serial) of its atoms plus one per ring
    # (a ring entity's atomi is 0)
    rec = c.rec
    chains = np.unique(rec["chain"])
    assert len(chains) == c.n_chains and rec["chain"].tolist() == sorted(rec["chain"].tolist())  # (file order = name order: chain ranks agree either way)
    keys = np.unique(np.rec.fromarrays([rec["chain"], rec["resi"], rec["altloc"], rec["serial"]], names="c,r,a,s"))
    per_chain, ents = np.unique(keys["c"], return_counts=True)
    ents[per_chain == b"A"] += 1
    assert int(ents.max()) - 1 == c.max_ent_rank
    assert c.any_icode == bool((rec["icode"] != b"").any())
    p = c.plan()
    if c.widths:
        assert (p["model_bits"], p["chain_bits"], p["rank_bits"]) == c.widths


def test_tie_runs_are_decided_at_every_level():
    """Inside a run the oracle orders by (from_insertion, to_insertion, distance); neighbours of a run differ in the from code alone, in the to code with
    equal from codes, and in the distance alone -- there by ONE f32 ulp, which survives the narrowing -- and no two rows agree in all three."""
    for name, c in CASES.items():
        if c.tie_run < 2:
            continue
        rows = tec.oracle_rows(name, "/")
        (lo, n), = [(lo, n) for lo, n in runs(rows) if n == c.tie_run]
        run = rows[lo:lo + n]
        trip = list(zip(run["from"]["insertion"].tolist(), run["to"]["insertion"].tolist(), run["distance"].astype(np.float32).tolist()))
        assert trip == sorted(trip) and len(set(trip)) == n, name
        level = {"from": 0, "to": 0, "dist": 0}
        for a, b in zip(trip, trip[1:]):
            level["from" if a[0] != b[0] else "to" if a[1] != b[1] else "dist"] += 1
        assert level["dist"] == 1 and (n < 63 or (level["from"] >= 5 and level["to"] >= 20)), (name, level)
        (k,) = [k for k in range(n - 1) if trip[k][:2] == trip[k + 1][:2]]
        d0, d1 = np.float32(trip[k][2]), np.float32(trip[k + 1][2])
        assert d0 == np.float32(tec.D_ONE) and d1 == np.nextafter(d0, np.float32(4.0)), name
        # the emitter's order is not the table's: the file lists the residues in falling code order
        file_order = [t for t in zip(c.rec["icode"][c.rec["chain"] == b"C"].tolist())]
        assert file_order != sorted(file_order) or n == 2, name


def test_the_straddling_run_crosses_the_block_edge():
    c = CASES["tie_63_straddles_256"]
    assert c.run_start < 255 and c.run_start + c.tie_run > 257 and c.pairs > tec.SMALL_PAIRS  # k_tie_fix: blocks of 256 sorted positions


def test_routes_by_hand():
    """route() against the expectation the issue names, for the cases where it names one."""
    r = lambda name, bits=0: CASES[name].route(bits)
    pick = lambda d, *keys: tuple(d[k] for k in keys)
    assert pick(r("rows_0_no_pairs"), "table_small", "table_plan", "table_pairs") == (0, 0, 0)
    assert pick(r("rows_4096"), "table_small", "table_plan") == (0, 0)
    assert pick(r("rows_4097_fallback"), "table_small", "table_plan", "table_long_way") == (1, 6, 0)
    assert pick(r("pairs_2048"), "table_small", "table_plan") == (0, 0) and pick(r("pairs_2049"), "table_small", "table_plan") == (-1, 6)
    for L in tec.TIE_RUNS:
        assert pick(r(f"tie_{L}_small"), "table_small", "table_plan", "table_long_way") == ((0, 0, 0) if L < 64 else (2, 6, 1)), L
        assert pick(r(f"tie_{L}_general"), "table_small", "table_plan", "table_long_way") == (-1, 6, int(L >= 64)), L
    assert pick(r("width_64_small"), "table_small", "table_plan") == (0, 0)
    assert pick(r("width_66_refused"), "table_small", "table_plan") == (4, 6)
    assert pick(r("width_plan_25"), "table_small", "table_plan") == (-1, 25)
    assert pick(r("ring_reserve_1088"), "table_small", "table_ring_rows", "table_ring_cap") == (0, 1088, 1088)
    assert pick(r("ring_reserve_1089"), "table_small", "table_ring_rows", "table_ring_cap") == (0, 1089, 1089)
    assert pick(r("ring_reserve_1089_general"), "table_small", "table_plan", "table_ring_cap") == (-1, 6, 1089)
    assert pick(r("rows_65"), "table_ring_cap") == (1088,)
    for name in tec.FORCED_CASES:
        c = CASES[name]
        for digits, bits in tec.forced(c).items():
            assert 6 <= bits <= 64
            got = c.route(bits)
            assert (got["table_small"], got["table_plan"], got["table_long_way"]) == (4 if c.pairs <= tec.SMALL_PAIRS else -1, digits, int(c.tie_run >= 64)), (name, digits)
