"""The table plan (arpeggia_amd/csrc/table_plan.h plan_table) on the CPU: tests/table_plan/plan_dump.cpp, a stand-alone host program that includes nothing
but that header, answers queries.  Expected plans are written out by hand at every width test's limit and one bit beyond, with and without the knob
table_key_bits, and swept against the plain restatement of tests/table_edge_cases.py (plan)."""
import subprocess
from pathlib import Path

import pytest

import table_edge_cases as tec
from arpeggia_amd.build import CSRC, hipcc


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = tmp_path_factory.mktemp("table_plan") / "plan_dump"
    # (hipcc as a plain C++17 host compiler: no HIP header, no device pass)
    r = subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-command-line-argument", f"-I{CSRC}",
                        str(Path(__file__).resolve().parent / "table_plan" / "plan_dump.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args, stdin=""):
        r = subprocess.run([str(exe), *args], input=stdin, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def plans(dump, queries):
    """queries: (n_pairs, n_models, n_chains, max_ent_rank, any_icode, key_bits)."""
    out = dump(stdin="".join("%d %d %d %d %d %d\n" % tuple(int(v) for v in q) for q in queries))
    assert len(out) == len(queries)
    res = []
    for line in out:
        head, rest = line.split(" P")
        general, long_way = rest.split(" L")
        h = [int(v) for v in head.split()]
        pairs_of = lambda s: [(int(a), int(b)) for a, b in zip(s.split()[0::2], s.split()[1::2])]
        res.append({"small_try": bool(h[0]), "few_pairs": bool(h[1]), "keys_fit_small": bool(h[2]), "model_bits": h[3], "chain_bits": h[4], "rank_bits": h[5], "limit": h[6],
                    "digits": h[7], "passes": pairs_of(general), "long_way": pairs_of(long_way)})
    return res


def plan(dump, pairs=100, models=1, chains=1, max_rank=0, icode=0, key_bits=0):
    return plans(dump, [(pairs, models, chains, max_rank, icode, key_bits)])[0]


def test_constants(dump):
    c = {k: int(v) for k, v in (line.split() for line in dump("constants"))}
    assert c == {"kSmallRows": 4096, "kSmallThreads": 1024, "kSmallIdxBits": 12, "kSmallPairs": 2048, "kTableMinKeyBits": 6, "kTableMaxKeyBits": 64}
    assert (tec.SMALL_ROWS, tec.SMALL_PAIRS, tec.SMALL_IDX_BITS) == (c["kSmallRows"], c["kSmallPairs"], c["kSmallIdxBits"])


def test_widths(dump):
    """Bits that hold 0 .. v - 1: one at least, 32 at most."""
    for chains, bits in ((0, 1), (1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (2048, 11), (2049, 12), (16384, 14), (16385, 15), (2 ** 31, 31), (2 ** 31 + 1, 32), (2 ** 40, 32)):
        p = plan(dump, chains=chains, models=chains)
        assert (p["chain_bits"], p["model_bits"]) == (bits, bits), chains
    for max_rank, bits in ((0, 1), (1, 1), (2, 2), (3, 2), (4, 3), (2047, 11), (2048, 12), (2 ** 32 - 1, 32)):
        assert plan(dump, max_rank=max_rank)["rank_bits"] == bits, max_rank


def test_pair_limit(dump):
    assert [plan(dump, pairs=n)["small_try"] for n in (0, 1, 2047, 2048, 2049, 10 ** 9)] == [True, True, True, True, False, False]


def test_every_width_test_at_its_limit_and_one_beyond(dump):
    # one model: 1 + 2 c + 2 r + 5 (+ 12 for the one-launch word) against 64
    # the one-launch word: c = 11, r = 12 is 64 (the last that fits), c = 12, r = 12 is 66, c = 11, r = 13 is 66; two models keep 1 bit, three take 2: 65
    at = plan(dump, chains=2048, max_rank=2048)
    assert (at["chain_bits"], at["rank_bits"], at["small_try"], at["passes"]) == (11, 12, True, [(6, 52)])
    assert not plan(dump, chains=2049, max_rank=2048)["small_try"] and not plan(dump, chains=2048, max_rank=4096)["small_try"]
    assert plan(dump, chains=2048, max_rank=2048, models=2)["small_try"] and not plan(dump, chains=2048, max_rank=2048, models=3)["small_try"]
    # one merged key: c = 14, r = 15 is 1 + 28 + 30 + 5 = 64: pass 6; r = 16 is 66, and three models 65: passes 2 and 5
    assert plan(dump, pairs=5000, chains=16384, max_rank=2 ** 15 - 1)["passes"] == [(6, 64)]
    assert plan(dump, pairs=5000, chains=16384, max_rank=2 ** 15)["passes"] == [(2, 21), (5, 45)]
    assert plan(dump, pairs=5000, chains=16384, max_rank=2 ** 15 - 1, models=3)["passes"] == [(2, 20), (5, 45)]
    assert plan(dump, pairs=5000, chains=16385, max_rank=16384)["passes"] == [(2, 20), (5, 46)]  # (the natural case of tests/table_edge_cases.py)
    # two passes: m + 2 c + r <= 64: m = 16 (65 536 models), c = 14, r = 20 is 64; r = 21, or c = 15 (66), or 65 537 models (17 bits), is beyond: passes 2, 3, 4
    assert plan(dump, models=65536, chains=16384, max_rank=2 ** 20 - 1)["passes"] == [(2, 25), (5, 64)]
    assert plan(dump, models=65536, chains=16384, max_rank=2 ** 20)["passes"] == [(2, 26), (3, 21), (4, 44)]
    assert plan(dump, models=65537, chains=16384, max_rank=2 ** 20 - 1)["passes"] == [(2, 25), (3, 20), (4, 45)]
    assert plan(dump, models=65536, chains=16385, max_rank=2 ** 20 - 1)["passes"] == [(2, 25), (3, 20), (4, 46)]


def test_long_way(dump):
    """The tie-breaking keys in front of the same passes: distance (32 bits), the insertion codes (64) only where an atom carries one."""
    for kw in (dict(chains=3, max_rank=99), dict(pairs=5000, chains=16385, max_rank=16384), dict(models=65537, chains=16384, max_rank=2 ** 20)):
        for icode in (0, 1):
            p = plan(dump, icode=icode, **kw)
            assert p["long_way"] == [(0, 32)] + ([(1, 64)] if icode else []) + p["passes"]
            assert p["digits"] == int("".join(str(a) for a, _ in p["passes"]))


def test_knob(dump):
    """table_key_bits stands for the 64 of all three tests and moves the plan only: every pass keeps the real width of its key."""
    kw = dict(chains=1, max_rank=600)  # 1ubq-like: 1 + 2 + 2 x 10 + 5 = 28 bits, 40 with the row index, 13 for pass 5
    assert plan(dump, **kw)["limit"] == 64 and plan(dump, key_bits=40, **kw)["limit"] == 40
    assert [plan(dump, key_bits=v, **kw)["small_try"] for v in (0, 64, 40, 39)] == [True, True, True, False]
    assert [plan(dump, key_bits=v, **kw)["passes"] for v in (40, 28)] == [[(6, 28)]] * 2
    assert [plan(dump, key_bits=v, **kw)["passes"] for v in (27, 13)] == [[(2, 15), (5, 13)]] * 2
    assert [plan(dump, key_bits=v, **kw)["passes"] for v in (12, 6)] == [[(2, 15), (3, 10), (4, 3)]] * 2
    assert [int(v) for v in dump("valid", stdin="-1 0 1 5 6 7 63 64 65 4096\n")] == [0, 1, 0, 0, 1, 1, 1, 1, 0, 0]


def test_sweep_against_the_restatement(dump):
    sizes = [0, 1, 2, 3, 2048, 2049, 16384, 16385, 65536, 65537, 2 ** 20, 2 ** 31, 2 ** 32 - 1]
    qs = [(pairs, m, c, r, ic, kb) for pairs in (0, 2048, 2049) for m in sizes[:-1] for c in sizes[:-1] for r in sizes for ic in (0, 1) for kb in (0, 6, 28, 52)]
    digits = set()
    for q, p in zip(qs, plans(dump, qs)):
        assert p == tec.plan(*q), q
        assert all(0 < end <= 64 + 32 for _, end in p["passes"])
        assert p["small_try"] <= (p["passes"][0][0] == 6), q  # the one-launch word holds the merged key: never tried where pass 6 does not exist
        digits.add(p["digits"])
    assert digits == {6, 25, 234}


def test_knob_and_route_record_through_the_library():
    """arp_debug_set refuses what table_key_bits_valid refuses; arp_debug_get knows the seven keys of the route record and nothing else (no device needed)."""
    import arpeggia_amd as aa

    try:
        for bad in (-1, 1, 5, 65, 2 ** 40):
            with pytest.raises(aa.ArpeggiaError):
                aa.debug_set("table_key_bits", bad)
        for ok in (6, 13, 64, 0):
            aa.debug_set("table_key_bits", ok)
    finally:
        aa.debug_set("table_key_bits", 0)
    for key in ("table_small", "table_pairs", "table_atom_rows", "table_ring_rows", "table_plan", "table_long_way", "table_ring_cap"):
        assert isinstance(aa.debug_get(key), int)
    for key in ("table", "table_key_bits", "timing", ""):
        with pytest.raises(aa.ArpeggiaError):
            aa.debug_get(key)
