"""The device contact table at its row, tie-run, key-width and ring-reserve edges: the built cases of tests/table_edge_cases.py (each reaches its edge by
construction: tests/test_table_edges_host.py) through arp_get_contacts, row for row against the oracle's table -- strings and order exact, floats within
the suite's DIST_TOL / ANGLE_TOL_DEG (under a forced key width also byte for byte against the unforced device table) -- and the route the call took (arp_debug_get "table_*") against the case's expectation, exactly.  Every case runs
through each of its chain-group specs, twice in a row.  The knob table_key_bits is process-wide: the tests that set it restore it in a finally."""
import time

import numpy as np
import pytest

import arpeggia_amd as aa
import synth
import table_edge_cases as tec
from test_gpu_parity import _lines_close, _table_lines

pytestmark = pytest.mark.gpu

CASES = tec.all_cases()
ROUTE_KEYS = ("table_small", "table_pairs", "table_atom_rows", "table_ring_rows", "table_plan", "table_long_way", "table_ring_cap")


@pytest.fixture(scope="module")
def ctx():
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


@pytest.fixture(scope="module")
def structures():
    made = {}

    def get(name):
        if name not in made:
            made[name] = aa.load_model(str(synth.DATA / "1ubq.pdb")) if name == "1ubq" else aa.Structure.from_records(CASES[name].rec)
        return made[name]
    return get


def route():
    return {k: aa.debug_get(k) for k in ROUTE_KEYS}


def check(ctx, s, name, groups, want_route, repeats=2):
    want = tec.oracle_lines(name, groups)
    for _ in range(repeats):
        t0 = time.perf_counter()
        cols = ctx.get_contacts(s, groups, tec.VDW_COMP, tec.CUTOFF)
        dt = time.perf_counter() - t0
        got_route = route()
        print(f"{name} {groups}: {len(cols['model'])} rows in {dt * 1e3:.2f} ms, route {got_route}")
        _lines_close(_table_lines(cols), want)
        assert got_route == want_route, (name, groups)
    return cols


def assert_same_bytes(got, want, what):
    """Every column of two tables: same names, types, lengths and bytes."""
    assert sorted(got) == sorted(want), what
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_oracle_and_takes_its_route(ctx, structures, name):
    c = CASES[name]
    for groups in c.groups:
        check(ctx, structures(name), name, groups, c.route())


def test_route_record_and_knob_interface():
    with pytest.raises(aa.ArpeggiaError):
        aa.debug_get("table_nothing")
    try:
        for bad in (-1, 1, 5, 65):
            with pytest.raises(aa.ArpeggiaError):
                aa.debug_set("table_key_bits", bad)
        for ok in (6, 64):
            aa.debug_set("table_key_bits", ok)
    finally:
        aa.debug_set("table_key_bits", 0)


@pytest.mark.parametrize("name", tec.FORCED_CASES)
@pytest.mark.parametrize("digits", [6, 25, 234])
def test_forced_key_widths_change_the_plan_not_the_table(ctx, structures, name, digits):
    """table_key_bits moves the plan through {6}, {2, 5} and {2, 3, 4} (the last is out of reach of any input a test can afford: it needs some 65 537
    models in 16 385 chains): passes 3 and 4, and k_tie_fix comparing rows without the merged key.  The table is the unforced one, byte for byte."""
    c = CASES[name]
    bits = tec.forced(c)[digits]
    try:
        aa.debug_set("table_key_bits", 0)
        unforced = check(ctx, structures(name), name, "/", c.route(), repeats=1)
        aa.debug_set("table_key_bits", bits)
        want = c.route(bits)
        assert want["table_plan"] == digits
        for _ in range(2):
            assert_same_bytes(check(ctx, structures(name), name, "/", want, repeats=1), unforced, (name, digits, bits))
    finally:
        aa.debug_set("table_key_bits", 0)


@pytest.mark.parametrize("digits", [6, 25, 234])
def test_forced_key_widths_on_1ubq(ctx, structures, digits):
    try:
        aa.debug_set("table_key_bits", 0)
        unforced = ctx.get_contacts(structures("1ubq"), "/", tec.VDW_COMP, tec.CUTOFF)
        assert (aa.debug_get("table_small"), aa.debug_get("table_plan")) == (0, 0)  # 532 rows: the one-launch path when nothing is forced
        _lines_close(_table_lines(unforced), tec.oracle_lines("1ubq", "/"))
        aa.debug_set("table_key_bits", tec.UBQ_FORCED[digits])
        for _ in range(2):
            cols = ctx.get_contacts(structures("1ubq"), "/", tec.VDW_COMP, tec.CUTOFF)
            r = route()
            _lines_close(_table_lines(cols), tec.oracle_lines("1ubq", "/"))
            assert (len(cols["model"]), r["table_small"], r["table_plan"], r["table_long_way"], r["table_atom_rows"] + r["table_ring_rows"]) == (532, 4, digits, 0, 532)
            assert_same_bytes(cols, unforced, ("1ubq", digits))
    finally:
        aa.debug_set("table_key_bits", 0)


def test_routes_in_sequence_on_one_context(structures):
    """One-launch, general, one-launch with fallback, an empty table, one-launch with ring rows, the ring-row repeat, 1ubq -- forwards and backwards on ONE
    fresh context: the landing buffer and the second scratch slot change size between the routes, and the empty table finds other structures' rows there."""
    c = aa.Context(0)
    for name in tec.SEQUENCE + tec.SEQUENCE[::-1]:
        if name == "1ubq":
            cols = c.get_contacts(structures(name), "/", tec.VDW_COMP, tec.CUTOFF)
            _lines_close(_table_lines(cols), tec.oracle_lines(name, "/"))
            assert (aa.debug_get("table_small"), aa.debug_get("table_plan"), aa.debug_get("table_atom_rows") + aa.debug_get("table_ring_rows")) == (0, 0, 532)
        else:
            check(c, structures(name), name, "/", CASES[name].route(), repeats=1)
