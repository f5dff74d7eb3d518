"""Pair lists of the product against the oracle's, for the GPU tests that compare whole lists bit for bit."""
from __future__ import annotations

import numpy as np

import arpeggia_amd as aa
import oracle_binding as ob
import synth


def canon(p):
    return p[np.lexsort((p["j"], p["i"]))]


def assert_same_as_oracle(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} pairs vs oracle {len(want)}"
    g, w = canon(got), canon(want)
    assert np.array_equal(g["i"], w["i"].astype(np.uint32)) and np.array_equal(g["j"], w["j"].astype(np.uint32)), f"{what}: pair indices differ"
    assert np.array_equal(g["kind"], w["kind"]), f"{what}: kinds differ"
    assert np.array_equal(g["dist"], w["dist"].astype(np.float32)), f"{what}: f32 distances not bit-identical"


def both(rec: dict, groups: str = "/"):
    """The product's SoA of the records and the oracle's list of all candidates (vdw_comp 0.1, cutoff 6.5)."""
    soa = aa.Structure.from_records(rec, hierarchy=True).soa(groups)
    want = ob.Structure.from_atoms(synth.records_to_oracle(rec, flat=True), flat=True).atomic_contacts(groups, 0.1, 6.5)
    return soa, want
