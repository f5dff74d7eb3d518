"""Contact frequencies across frames (arp_contact_frequencies) at the edges of its kernels and of its host loop: the cases of
tests/freq_edge_cases.py on the device.

Every case compares the whole returned table -- aa.FREQ_COLUMNS plus from_atom / to_atom, row order included, distances for exact equality --
with the closed-form reference of the schedule, after asserting from the layout prediction that the case still reaches the edge it is named
for (runs against lanes, waves and blocks of k_freq_reduce; the wave prefix and the tail wave of k_freq_expand; the skipped passes of the host
loop; the grow-and-repeat path with and without an aggregate to keep; the sort's last key bit; the cap of 65 535 frames per pass; the
rounding of frequency).  tests/test_freq_edge_host.py pins the reference to the oracle on the CPU.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import freq_edge_cases as fe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    aa.debug_set("freq_chunk_atoms", 0)
    aa.debug_set("freq_cap_items", 0)


def to_bytes(t: dict) -> bytes:
    return b"".join(np.ascontiguousarray(t[c]).tobytes() for c in sorted(t))


def run(ctx, name: str, cap: int | None = None) -> dict:
    """The case on the device with its pass size and (cap None) its own freq_cap_items, after the case's reach assertions."""
    fe.check_reach(name)
    c = fe.cases()[name]
    assert [k for k, _ in aa.FREQ_COLUMNS] + ["from_atom", "to_atom"] == fe.COLUMNS
    s = aa.Structure.from_records(c.top.rec)
    assert s.n_atoms == c.top.n
    aa.debug_set("freq_chunk_atoms", c.chunk_atoms)
    aa.debug_set("freq_cap_items", c.cap if cap is None else cap)
    return ctx.contact_frequencies(s, fe.frames(c.top, c.D), "/", fe.VDW_COMP, fe.CUTOFF)


def check(ctx, name: str) -> dict:
    got = run(ctx, name)
    fe.assert_same_table(got, fe.reference_of(name))
    return got


RUN_CASES = [n for n in fe.cases() if n.startswith("runs_")]


@pytest.mark.parametrize("name", RUN_CASES)
def test_runs_against_lanes_waves_and_blocks(ctx, name):
    """One pass (or the second pass of two, every run then carrying its aggregate item) whose sorted items form runs of chosen lengths at
    chosen lanes: k_freq_reduce's segmented fold and its one atomic per run and wave."""
    check(ctx, name)


def test_across_passes(ctx):
    """Keys that come and go over five passes: first frame only, last frame only, a pass without the key, new in the last pass, every frame,
    extremes in the first and last pass, equal extremes, two codes of one motif with different counts."""
    got = check(ctx, "across_keys")
    assert (got["frequency"] == 1.0).sum() == 1


@pytest.mark.parametrize("name", ["skip_middle", "skip_first_apart_k0", "skip_first_k0_apart"])
def test_skipped_passes(ctx, name):
    """Passes without candidate pairs and passes whose candidates all have kind == 0 (none listed), in the middle and in front of a call:
    the buffers are first allocated in pass 2 when the first two passes are of these kinds."""
    assert len(check(ctx, name)["n_frames"]) > 0


def test_only_skipped_passes(ctx):
    got = check(ctx, "skip_all")
    assert set(got) == set(fe.COLUMNS) and all(len(v) == 0 for v in got.values())


def test_expand_mixed_pairs(ctx):
    """k_freq_expand on a pair list of pairs with 1 and 2 set bits and a partly filled tail wave (its 0-bit lanes), among candidates the pair
    pass drops; coincident atoms give 0.0 exactly."""
    got = check(ctx, "expand_mixed")
    clash = got["interaction"] == 0
    assert clash.any() and (got["min_distance"][clash] == 0.0).all()


@pytest.mark.parametrize("name", ["capacity_1", "capacity_exact"])
def test_capacity_knob(ctx, name):
    """freq_cap_items: buffers that grow in the first pass (nothing to keep) and in later passes (the aggregate moves), or that fit pass 0
    exactly and miss pass 1 by one item.  Rows that exist only in the aggregate when the buffers grow come back intact; the bytes are those of
    the run without the knob."""
    got = check(ctx, name)
    assert to_bytes(run(ctx, name, cap=0)) == to_bytes(got)


def test_capacity_floor(ctx):
    """The first allocation of 65 536 items outgrown by a later pass, without the knob."""
    check(ctx, "capacity_floor")


@pytest.mark.parametrize("n", [64, 65, 128, 129])
def test_key_bits(ctx, n):
    """The sort's end bit at n = 2^k and 2^k + 1 atoms: the row from atom n - 1 comes last."""
    got = check(ctx, f"key_bits_{n}")
    assert got["from_atom"][-1] == n - 1


def test_many_frames(ctx):
    """70 000 frames of four atoms: two passes under the cap of 65 535 frames per pass."""
    check(ctx, "many_frames")


@pytest.mark.parametrize("F", [1, 3, 7, 2000])
def test_frequency_rounding(ctx, F):
    got = check(ctx, f"rounding_{F}")
    assert np.array_equal(got["frequency"], (got["n_frames"].astype(np.float64) / F).astype(np.float32))


@pytest.mark.parametrize("name", ["runs_second_pass_BA", "across_keys"])
def test_per_frame_device_pairs_agree(ctx, name):
    """The table that tests/test_freq_gpu.py builds from one Context.atomic_contacts call per frame equals the closed form too: a disagreement
    between the device table and the closed form then lies in the frequency kernels, not in the pair pass."""
    from test_freq_gpu import expected

    c = fe.cases()[name]
    s = aa.Structure.from_records(c.top.rec)
    fe.assert_same_table(expected(ctx, s, fe.frames(c.top, c.D), "/"), fe.reference_of(name))
