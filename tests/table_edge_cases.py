"""Built cases for the edges of the device contact table (arpeggia_amd/csrc/table_dev.hip device_table, table_plan.h): row counts around the
one-launch kernel's words-per-thread steps and its 4096-row limit, the 2048-pair limit, tie runs around the 63 rows k_tie_fix resolves in place,
key widths around the 64-bit key word, and the ring-row reserve.  No product imports: tests/test_table_edges_host.py checks on the CPU that the
oracle's table of every case has the closed-form counts, tie run and key widths named here (so every case reaches its edge by construction),
tests/test_table_edges_gpu.py runs the cases on the device and compares the table with the oracle's and the route record with route().

Every case is one PHE ring at the origin (chain A, residue 1: the table refuses a ring-free model) plus isolated pieces on a plane, 40 A apart,
100 A from the ring:

  motif      LYS NZ (one chain) ... ASP OD1 (another chain), each atom a residue of its own.  The distance alone chooses the rows
             (vdw_comp 0.1, cutoff 6.5; pinned by the oracle in the host test), every distance at least 0.05 A from a rule's threshold:
               "two"   2.95 A   IonicBond + VanDerWaalsContact     "one"   3.5 A   IonicBond     "none"   4.7 A   a candidate pair, no row
             The table's pair pass runs contacts-only, so a "none" motif adds nothing to the pair count the table sees.
  cations    m NZ atoms of ONE LYS residue (chain B, residue 1) above the ring, on an 11 x 11 grid of 0.2 A steps at z = 3.6 .. 4.0 A in 0.05 A
             steps: m CationPi rows from the ring, no atom rows.  One ring reserves 64 + 1024 = 1088 ring rows.
  tie run    rows that agree in all ten sort keys (model, chains, resi, altloc, atomi of both ends, interaction): "one" motifs whose atoms all
             carry resi 10 and serial 5 in chains C (NZ) and D (OD1 / OD2) and differ in the insertion code only.  The oracle orders them by
             (from_insertion, to_insertion, distance).  A run of L rows = one LYS NZ with OD1 at 3.5 A and OD2 one f32 ulp further away on the
             other side (both insertion codes equal: the distance decides) + L - 2 motifs over a 13 x 11 grid of code pairs drawn in a scrambled
             order (several share the from code: the to code decides; the rest differ in the from code).  No two rows of a run agree in all three.
             Atoms of one (chain, resi, insertion code) are adjacent in the file: one residue each, with as many NZ (or OD1) atoms as motifs use it.
  fillers    "one" motifs in chains A -> B (they sort before the run) and E -> F (behind it): they set the run's sorted position and the pair count.
  chains     key-width cases: every OD1 in a chain of its own (zero-padded names, so that file order = name order), all NZ in chain A.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import synth

CUTOFF, VDW_COMP = 6.5, 0.1
SPACING, FIRST_SITE = 40.0, 100.0
D_TWO, D_ONE, D_NONE = 2.95, 3.5, 4.7
ULP_AT_3_5 = 2.0 ** -22  # one f32 ulp in [2, 4)
RING_NAMES = ("CG", "CD1", "CD2", "CE1", "CE2", "CZ")
CODES = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
TIE_RESI, TIE_SERIAL = 10, 5
# device_table's constants (table_plan.h; tests/test_table_plan_host.py pins them)
SMALL_ROWS, SMALL_PAIRS, SMALL_IDX_BITS, TIE_RUN = 4096, 2048, 12, 64


def width(v: int) -> int:
    """Bits that hold 0 .. v - 1 (at least one, at most 32)."""
    b = 1
    while b < 32 and (1 << b) < v:
        b += 1
    return b


def plan(pairs: int, n_models: int, n_chains: int, max_ent_rank: int, any_icode: bool, key_bits: int = 0) -> dict:
    """plan_table (table_plan.h) restated: three width tests against the key word (64 bits, or what the knob table_key_bits says)."""
    limit = key_bits or 64
    mb, cb, rb = width(max(n_models, 1)), width(max(n_chains, 1)), width(max_ent_rank + 1)
    top = mb + 2 * cb
    every = top + 2 * rb + 5
    if every <= limit:
        passes = [(6, every)]
    elif top + rb <= limit:
        passes = [(2, rb + 5), (5, top + rb)]
    else:
        passes = [(2, rb + 5), (3, rb), (4, top)]
    long_way = [(0, 32)] + ([(1, 64)] if any_icode else []) + passes
    return {"small_try": pairs <= SMALL_PAIRS and every + SMALL_IDX_BITS <= limit, "few_pairs": pairs <= SMALL_PAIRS, "keys_fit_small": every + SMALL_IDX_BITS <= limit,
            "model_bits": mb, "chain_bits": cb, "rank_bits": rb, "limit": limit, "digits": int("".join(str(p) for p, _ in passes)), "passes": passes, "long_way": long_way}


@dataclass
class Case:
    name: str
    rec: dict
    pairs: int        # contact pairs (kind != 0)
    atom_rows: int
    ring_rows: int
    tie_run: int      # the longest run of rows that agree in the ten sort keys (1: none tie)
    groups: tuple     # chain-group specs the case runs through; the counts hold for each
    n_chains: int
    max_ent_rank: int
    any_icode: bool
    run_start: int = -1   # sorted position of the tie run's first row where the case places it (-1: not pinned)
    widths: tuple = field(default=())  # (model_bits, chain_bits, rank_bits) where the case names them

    @property
    def rows(self) -> int:
        return self.atom_rows + self.ring_rows

    def plan(self, key_bits: int = 0) -> dict:
        return plan(self.pairs, 1, self.n_chains, self.max_ent_rank, self.any_icode, key_bits)

    def route(self, key_bits: int = 0) -> dict:
        """The route record (arp_debug_get "table_*") this case must leave, from device_table as read: the one-launch kernel first gives up on
        ring rows beyond the reserve (the call reserves what was counted and repeats, once), then on more than 4096 rows (status 1), then on a tie
        run of 64 or more (status 2); the general path sorts by the plan's passes, and a second time the long way after such a run."""
        p = self.plan(key_bits)
        reserve = 64 * 1 + 1024
        ring_cap = max(reserve, self.ring_rows)
        if not p["few_pairs"]:
            small = -1
        elif not p["keys_fit_small"]:
            small = 4
        elif self.rows > SMALL_ROWS:
            small = 1
        elif self.tie_run >= TIE_RUN:
            small = 2
        else:
            small = 0
        general = small != 0
        return {"table_small": small, "table_pairs": self.pairs, "table_atom_rows": self.atom_rows, "table_ring_rows": self.ring_rows,
                "table_plan": p["digits"] if general and self.rows else 0, "table_long_way": int(general and self.tie_run >= TIE_RUN), "table_ring_cap": ring_cap}


class _Builder:
    def __init__(self):
        self.cols = {k: [] for k in ("x", "y", "z", "occupancy", "serial", "resi", "name", "resn", "chain", "altloc", "icode", "element", "model_serial")}
        self.site = 0
        self.side = 1

    def add(self, resn, name, elem, chain, resi, xyz, icode="", serial=None):
        k = len(self.cols["x"])
        for c, v in (("x", xyz[0]), ("y", xyz[1]), ("z", xyz[2]), ("occupancy", 1.0), ("serial", k + 1 if serial is None else serial), ("resi", resi), ("name", name),
                     ("resn", resn), ("chain", chain), ("altloc", ""), ("icode", icode), ("element", elem), ("model_serial", 0)):
            self.cols[c].append(v)

    def next_site(self):
        s, self.site = self.site, self.site + 1
        return np.array([FIRST_SITE + SPACING * (s % self.side), SPACING * (s // self.side), 0.0])


def cation_points(m: int) -> np.ndarray:
    assert 0 <= m <= 11 * 11 * 9
    pts = [(-1.0 + 0.2 * i, -1.0 + 0.2 * j, 3.6 + 0.05 * k) for k in range(9) for j in range(11) for i in range(11)]
    return np.array(pts[:m]).reshape(m, 3)


def tie_codes(L: int, seed: int = 11):
    """[(from code, to code, distance or None)]: the rows of a run of L; None = the two rows of the ulp motif (code pair A / A)."""
    assert 2 <= L <= 13 * 11 + 1
    grid = [(a, b) for a in CODES[:13] for b in CODES[:11]][1:]  # without ("A", "A"): the ulp motif's
    rng = np.random.default_rng(seed)
    pick = [grid[k] for k in rng.permutation(len(grid))[:L - 2]]
    dist = 3.35 + 0.6 * rng.permutation(max(L - 2, 1))[:L - 2] / max(L - 2, 1)  # distinct, scrambled, inside [3.35, 3.95]
    return [("A", "A", None)] + [(a, b, float(d)) for (a, b), d in zip(pick, dist)]


def compose(name: str, two: int = 0, one: int = 0, none: int = 0, cations: int = 0, tie: int = 0, before: int = 0, after: int = 0, chain_per_motif: bool = False,
            lone_chains: int = 0, widths: tuple = ()) -> Case:
    """two / one / none: motifs NZ (chain A) -> OD1 (chain B, or a chain of its own with chain_per_motif); before / after: "one" fillers A -> B / E -> F
    around a tie run of `tie` rows in chains C -> D; lone_chains: single far GLY CA atoms, each a chain of its own."""
    b = _Builder()
    motifs = two + one + none + before
    sites = motifs + after + (max(tie - 1, 0)) + lone_chains
    b.side = max(1, int(np.ceil(np.sqrt(max(sites, 1)))))
    # chain A: the ring, then every NZ of the A -> . motifs
    for k, nm in enumerate(RING_NAMES):
        ang = np.pi / 3 * k
        b.add("PHE", nm, "C", "A", 1, (1.39 * np.cos(ang), 1.39 * np.sin(ang), 0.0))
    kinds = [D_TWO] * two + [D_ONE] * one + [D_NONE] * none
    order = np.random.default_rng(3).permutation(len(kinds))  # the three kinds mixed along the file
    dists = [kinds[k] for k in order] + [D_ONE] * before
    a_sites = [b.next_site() for _ in dists]
    for k, s in enumerate(a_sites):
        b.add("LYS", "NZ", "N", "A", 2 + k, s)
    # chain B: the cation residue, then the motifs' partners
    for q in cation_points(cations):
        b.add("LYS", "NZ", "N", "B", 1, q)
    has_b = cations > 0 or (len(dists) > 0 and not chain_per_motif)
    n_chains = 1 + int(has_b)
    for k, (s, d) in enumerate(zip(a_sites, dists)):
        chain = f"B{k + 1:05d}" if chain_per_motif else "B"
        b.add("ASP", "OD1", "O", chain, 2 + k, s + (d, 0.0, 0.0))
    if chain_per_motif:
        n_chains += len(dists)
    rank = {"A": 6 + 1 + len(dists), "B": cations + (0 if chain_per_motif else len(dists))}  # entities per chain (the ring is one: its atomi is 0)
    # chains C, D: the tie run
    any_icode = tie > 0
    if tie:
        rows = tie_codes(tie)
        place = {k: b.next_site() for k in range(len(rows))}
        for code in sorted({a for a, _, _ in rows}, reverse=True):  # residues in falling code order: file order is not the table's order
            for k, (a, _, _) in enumerate(rows):
                if a == code:
                    b.add("LYS", "NZ", "N", "C", TIE_RESI, place[k], icode=a, serial=TIE_SERIAL)
        for code in sorted({t for _, t, _ in rows}, reverse=True):
            for k, (_, t, d) in enumerate(rows):
                if t != code:
                    continue
                if d is None:
                    b.add("ASP", "OD2", "O", "D", TIE_RESI, place[k] - (D_ONE + ULP_AT_3_5, 0.0, 0.0), icode=t, serial=TIE_SERIAL)
                    b.add("ASP", "OD1", "O", "D", TIE_RESI, place[k] + (D_ONE, 0.0, 0.0), icode=t, serial=TIE_SERIAL)
                else:
                    b.add("ASP", "OD1", "O", "D", TIE_RESI, place[k] + (d, 0.0, 0.0), icode=t, serial=TIE_SERIAL)
        n_chains += 2
        rank["C"] = rank["D"] = 1
    if after:
        e_sites = [b.next_site() for _ in range(after)]
        for k, s in enumerate(e_sites):
            b.add("LYS", "NZ", "N", "E", 2 + k, s)
        for k, s in enumerate(e_sites):
            b.add("ASP", "OD1", "O", "F", 2 + k, s + (D_ONE, 0.0, 0.0))
        n_chains += 2
        rank["E"] = rank["F"] = after
    for k in range(lone_chains):
        b.add("GLY", "CA", "C", f"G{k + 1:05d}", 1, b.next_site())
    n_chains += lone_chains
    pairs = two + one + before + after + (tie if tie else 0)  # (the ulp motif: one NZ, two pairs)
    atom_rows = 2 * two + one + before + after + tie
    groups = ("/",) if chain_per_motif else (("/", "A,C,E/B,D,F") if tie or after else (("/", "A/B") if has_b else ("/",)))
    return Case(name, synth._finish(b.cols), pairs, atom_rows, cations, max(tie, 1), groups, n_chains, max(rank.values()) - 1, any_icode,
                run_start=(before + cations) if tie else -1, widths=widths)


def _split(total: int) -> dict:
    """Atom rows -> motifs: a third of the motifs two-row ones up to 2048 rows, as many two-row ones as it takes beyond (pairs stay <= 2048)."""
    two = total // 3 if total <= 2048 else total - 2048
    return dict(two=two, one=total - 2 * two, none=3)


ROW_COUNTS = (0, 1, 63, 64, 65, 1024, 1025, 2048, 2049, 4095, 4096)
TIE_RUNS = (2, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def all_cases() -> dict:
    cases = [compose("rows_0_no_pairs")]
    cases.append(compose("rows_0_candidates_only", none=5))
    for t in ROW_COUNTS[1:]:
        cases.append(compose(f"rows_{t}", **_split(t)))
    for t in ROW_COUNTS[1:]:  # the same totals with ring rows in the mix (1: the one ring row and no atom row)
        m = min(t, 7)
        cases.append(compose(f"rows_{t}_with_ring_rows", cations=m, **_split(t - m)))
    cases.append(compose("rows_4097_fallback", two=2048, cations=1))  # 4096 atom rows + 1 ring row: status 1, then the general path
    cases.append(compose("pairs_2048", one=2048))
    cases.append(compose("pairs_2049", one=2049))
    for L in TIE_RUNS:
        cases.append(compose(f"tie_{L}_small", tie=L, before=40, after=30))
        cases.append(compose(f"tie_{L}_general", tie=L, before=100, after=2100))
    cases.append(compose("tie_63_straddles_256", tie=63, before=225, after=2100))  # rows 225 .. 287 of the sorted table: both sides of k_tie_fix's block edge
    # natural key widths: 1 model bit + 2 x chain bits + 2 x rank bits + 5 + 12 index bits against 64
    cases.append(compose("width_64_small", one=2042, chain_per_motif=True, lone_chains=5, widths=(1, 11, 12)))    # 2048 chains, chain A: 2049 entities
    cases.append(compose("width_66_refused", one=2042, chain_per_motif=True, lone_chains=6, widths=(1, 12, 12)))  # 2049 chains
    cases.append(compose("width_plan_25", one=16378, chain_per_motif=True, lone_chains=6, widths=(1, 15, 15)))    # 16385 chains, chain A: 16385 entities: 66 bits
    cases.append(compose("ring_reserve_1088", cations=1088, one=3))
    cases.append(compose("ring_reserve_1089", cations=1089, one=3))
    cases.append(compose("ring_reserve_1089_general", cations=1089, one=2049))
    out = {c.name: c for c in cases}
    assert len(out) == len(cases)
    return out


# (case, key_bits) through forced key widths: the table must not change, the plan must.  Values from the cases' own widths (checked in the host test).
def forced(case: Case) -> dict:
    """{plan digits: key_bits} that force the three plans of the general path on this case (the merged key fits its own width, a row index with it does not)."""
    p = case.plan()
    top = p["model_bits"] + 2 * p["chain_bits"]
    every = top + 2 * p["rank_bits"] + 5
    return {6: every, 25: every - 1, 234: top + p["rank_bits"] - 1}


FORCED_CASES = ("tie_63_general", "tie_65_general", "tie_63_small", "tie_65_small")
# 1ubq (532 rows: the one-launch path when nothing is forced): one model, one chain, 9 .. 11 rank bits, so 26 .. 30 key bits.  32 holds the merged key but
# not 12 index bits with it: {6} on the general path; 20 is {2, 5} for 7 .. 17 rank bits, 8 is {2, 3, 4} from 6 rank bits on
UBQ_FORCED = {6: 32, 25: 20, 234: 8}
# (the empty table behind larger ones: the one-launch kernel must not follow a row that an earlier call left in the scratch block)
SEQUENCE = ("rows_65", "pairs_2049", "rows_4097_fallback", "rows_0_no_pairs", "rows_1025_with_ring_rows", "ring_reserve_1089", "1ubq")


# ---- the reference: the oracle's table, once per (case, chain groups) and process ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_structure(name: str):
    import oracle_binding as ob

    if name == "1ubq":
        return ob.Structure.load(str(synth.DATA / "1ubq.pdb"))
    return ob.Structure.from_atoms(synth.records_to_oracle(all_cases()[name].rec, flat=False), flat=False)


@functools.lru_cache(maxsize=None)
def oracle_rows(name: str, groups: str = "/"):
    rows = oracle_structure(name).get_contacts(groups, VDW_COMP, CUTOFF)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def oracle_lines(name: str, groups: str = "/") -> tuple:
    import oracle_binding as ob

    return tuple(ob.rows_to_csv_lines(oracle_rows(name, groups)))
