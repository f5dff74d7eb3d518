"""The cases of tests/freq_edge_cases.py on the CPU: the closed-form reference (a) equals the oracle loop (b) exactly on every case, and the
layout prediction (c) shows that every case reaches the edge it is named for.  tests/test_freq_edge_gpu.py runs the same cases on the device."""
from __future__ import annotations

import numpy as np
import pytest

import freq_edge_cases as fe

NAMES = list(fe.cases())


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_equals_oracle(name):
    c = fe.cases()[name]
    if c.oracle_frames is None:
        fe.assert_same_table(fe.oracle_table(c.top, c.D), fe.reference_of(name))
    else:  # frames 0, F - 1, each pass's first and last frame, every 997th frame
        lay = c.layout()
        ends = {f for ps in lay for f in (ps.f0, ps.f0 + ps.frames - 1)}
        assert ends | {0, c.F - 1} <= set(c.oracle_frames.tolist()) and set(range(0, c.F, 997)) <= set(c.oracle_frames.tolist())
        D = c.D[c.oracle_frames]
        fe.assert_same_table(fe.oracle_table(c.top, D), fe.reference(c.top, D))


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_edge(name):
    fe.check_reach(name)


@pytest.mark.parametrize("name", ["expand_mixed", "skip_middle", "capacity_exact"])
def test_layout_pair_count_is_the_oracles(name):
    """The layout's pairs are the oracle's pairs with kind != 0 (what the contacts-only pair pass lists); its candidates are all of them."""
    c = fe.cases()[name]
    assert (int(fe.has_candidate(c.D).sum()), sum(ps.n_pairs for ps in c.layout())) == fe.oracle_pairs(c.top, c.D)


def test_motifs_are_isolated():
    """Motifs and lone atoms sit at least 20 A apart in every state, in the largest topologies the cases use."""
    from scipy.spatial import cKDTree

    for name in ("capacity_floor", "key_bits_129"):
        top = fe.cases()[name].top
        xyz = fe.frames(top, np.full((1, top.K), fe.APART))[0]
        near = cKDTree(xyz).query_pairs(20.0, output_type="ndarray")
        assert len(near) == top.K and (near[:, 0] >= top.pads).all()
        assert ((near[:, 0] - top.pads) // 2 == (near[:, 1] - top.pads) // 2).all()


def test_layout_of_a_hand_schedule():
    """layout() itself on a schedule small enough to work out by hand: 2 motifs, passes of 2 frames, buffers of 3 items."""
    top = fe.topology(["CC", "ON"], "AB")
    D = np.array([[3.0, 8.0], [4.0, 5.5], [8.0, 8.0], [8.0, 8.0], [5.5, 8.0], [5.5, 5.5], [3.0, 3.5]])
    lay = fe.layout(top, D, per=2, cap0=3)
    assert [(ps.n_pairs, ps.n_items, ps.n_agg, ps.skipped, ps.allocated, ps.cap, ps.grew, ps.cap_after) for ps in lay] == [
        (2, 3, 0, None, True, 3, False, 3), (0, 0, 2, "no_pairs", False, 3, False, 3), (0, 0, 2, "no_pairs", False, 3, False, 3),
        (2, 3, 2, None, False, 3, True, 6)]
    assert [(r.key, r.start, r.length, r.in_agg) for r in lay[0].runs] == [((0, 1, 3), 0, 1, False), ((0, 1, 18), 1, 2, False)]
    assert [(r.key, r.start, r.length, r.in_agg) for r in lay[3].runs] == [((0, 1, 3), 0, 2, True), ((0, 1, 18), 2, 2, True), ((2, 3, 4), 4, 1, False)]
    assert fe.run_edges(lay[0]) == {"single_at_lane0", "ragged_tail"}
