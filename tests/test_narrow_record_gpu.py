"""The narrow (32-byte) exact record of the single-pass emitter (arp_internal.h Xrec): index | tag word, the tag test of the
pair filter with its rare branch to the real residue keys, the index split and its wide-record fallback, chain groups and contacts-only lists.

The 12-wave k_emit kernels read the record on single inputs from 20 417 atoms (320 wave-tasks) on; the 4-wave kernels of smaller inputs and packs keep the
wide record.  Every list is compared with the oracle's: indices, kinds and f32 distances bit for bit.  arp_pair_rare_batches says how many
batches of the last pass decided on the real keys; arp_debug_set("index_bits", v) fixes the index width or keeps the wide record."""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import oracle_binding as ob
import synth
from oracle_lists import assert_same_as_oracle, both, canon

N_CLOUD = 1 << 15  # the last index is the largest a 15-bit index holds; 512 wave-tasks: a 12-wave kernel with the four-way task split


def tagged_cloud(n: int, modulus: int, two_chains: bool) -> dict:
    """gen_s2's jittered lattice (atoms i, i + 1 and i + 2 of the input order are lattice neighbours, 2.7 and 5.4 A apart) with hand-set residue
    ordinals: they never decrease along the input order, and consecutive atoms differ by 0, 1, M, M + 1, M - 1, M + 2, M - 2, then 2, 3 six times over, in turn
    (M = the tag modulus), so that pairs within the cutoff have ordinals 0, +-1, M, M +- 1, M +- 2 apart -- both signs, as either atom can be the
    home atom of the pair.  two_chains: the second half of the atoms is chain B with the first half's ordinals over again."""
    rec = synth.gen_s2(n)
    steps = np.array([0, 1, modulus, modulus + 1, modulus - 1, modulus + 2, modulus - 2] + [2, 3] * 6, dtype=np.int64)
    inc = steps[np.arange(n) % len(steps)]
    inc[0] = 0
    half = n // 2 if two_chains else n
    inc[half:half + 1] = 0
    ro = np.concatenate([np.cumsum(inc[:half]), np.cumsum(inc[half:]) if two_chains else np.zeros(0, dtype=np.int64)])
    if two_chains:
        ro[half:] = ro[:n - half]
        rec["chain"] = np.where(np.arange(n) < half, b"A", b"B").astype("S8")
    assert ro.max() < 2 ** 31  # (the oracle's ordinals are int32, and a positional index never gets there)
    new_res = np.concatenate([[1], (np.diff(ro) != 0) | (np.arange(1, n) == half)])
    # two atoms that share an ordinal are one residue: give it one name (gen_s2 draws every atom's residue name on its own)
    twin = np.flatnonzero(new_res == 0)
    for k in (twin, twin - 1):
        rec["resn"][k], rec["name"][k], rec["element"][k] = b"ALA", b"CB", b"C"
    rec["res_ord"] = ro.astype(np.uint32)
    rec["res_id"] = (np.cumsum(new_res) - 1).astype(np.uint32)
    return rec


def ordinal_gaps_within_cutoff(rec: dict, cutoff: float = 6.5) -> set:
    from scipy.spatial import cKDTree

    xyz = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    pairs = cKDTree(xyz).query_pairs(cutoff, output_type="ndarray")
    same = rec["chain"][pairs[:, 0]] == rec["chain"][pairs[:, 1]]
    ro = rec["res_ord"].astype(np.int64)
    return set(np.unique(np.abs(ro[pairs[same, 0]] - ro[pairs[same, 1]])).tolist())


@pytest.fixture(scope="module")
def ctx():
    assert aa.device_count() >= 1, "no gfx950 device: the product has no CPU fallback"
    return aa.Context(0)


@pytest.fixture()
def index_bits():
    """Sets arp_debug_set("index_bits", v) for the test and puts the default back."""
    try:
        yield lambda v: aa.debug_set("index_bits", v)
    finally:
        aa.debug_set("index_bits", 0)


@pytest.fixture(scope="module")
def clouds():
    """The tagged clouds (one chain, two chains) at 20 index bits = tag modulus 4096, and their oracle lists: computed once."""
    out = {}
    for two in (False, True):
        rec = tagged_cloud(21000, 4096, two)
        out[two] = (rec,) + both(rec)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("two_chains", [False, True])
def test_tag_aliasing(ctx, index_bits, clouds, two_chains):
    """Ordinals of atoms within the cutoff that differ by 0, +-1, the tag modulus, the modulus +- 1 and +- 2: the tag test proves nothing for the first two
    and for the aliases of them (M, M +- 1), the rare branch decides those on the real keys, and the list is the oracle's."""
    rec, soa, want = clouds[two_chains]
    M = 4096
    assert {0, 1, M - 2, M - 1, M, M + 1, M + 2} <= ordinal_gaps_within_cutoff(rec)
    index_bits(20)  # 12 tag bits: modulus 4096
    for only in (False, True):
        got = ctx.atomic_contacts(soa, aa.default_params(contacts_only=only))
        rare = ctx.rare_batches()
        assert_same_as_oracle(got, want[want["kind"] != 0] if only else want, f"tagged cloud, two_chains={two_chains}, only={only}")
        assert rare > 0, "no batch took the rare branch: the narrow record did not run, or the tags decided what they cannot"
    index_bits(-1)  # the wide record: the same list, no rare branch
    got = ctx.atomic_contacts(soa)
    assert ctx.rare_batches() == 0
    assert_same_as_oracle(got, want, f"tagged cloud on the wide record, two_chains={two_chains}")


@pytest.mark.gpu
def test_index_split(ctx, index_bits):
    """One cloud of 2^15 atoms four ways -- the narrow record as the launcher sizes it (15 index bits: the last index is the largest one they hold), the
    same width by the knob, 20 index bits (12 tag bits: other aliases, other batches on the rare branch), the wide record by the knob -- and with one
    more atom, which does not fit 15 bits and keeps the wide record."""
    rec = tagged_cloud(N_CLOUD, 4096, False)  # (ordinal gaps of 4096 and 4096 +- 1 alias at 12 tag bits and are told apart at 17)
    soa, want = both(rec)
    lists = {}
    rares = {}
    for what, v in (("auto", 0), ("wide", -1), ("15 bits", 15), ("20 bits", 20)):
        index_bits(v)
        lists[what] = canon(ctx.atomic_contacts(soa))
        rare = rares[what] = ctx.rare_batches()
        assert (rare == 0) == (what == "wide"), f"{what}: {rare} rare batches"
        assert_same_as_oracle(lists[what], want, what)
    assert all(np.array_equal(lists["auto"], lists[k]) for k in ("wide", "15 bits", "20 bits"))
    assert rares["20 bits"] > rares["15 bits"], "the knob's width did not reach the kernel"
    # one more atom, 1.3 A beside the last one, a residue of its own: index 2^15 does not fit 15 bits
    more = {k: np.concatenate([v, v[-1:]]) for k, v in rec.items()}
    more["x"][-1] += 1.3
    more["serial"][-1] += 1; more["resi"][-1] += 1; more["res_id"][-1] += 1; more["res_ord"][-1] += 5
    soa1, want1 = both(more)
    index_bits(15)
    tipped = canon(ctx.atomic_contacts(soa1))
    assert ctx.rare_batches() == 0, "an index that does not fit the split must keep the wide record"
    assert_same_as_oracle(tipped, want1, "one atom past 15 index bits")
    index_bits(0)
    again = canon(ctx.atomic_contacts(soa1))
    assert ctx.rare_batches() > 0
    assert np.array_equal(tipped, again)
    both_below = (tipped["i"] < N_CLOUD) & (tipped["j"] < N_CLOUD)
    assert np.array_equal(tipped[both_below], lists["auto"])  # the pairs among the first 2^15 atoms are the first cloud's


@pytest.mark.gpu
def test_chain_groups_and_contacts_only(ctx):
    """Chain groups other than "/" decide every batch on the real keys (the tags only serve the all-in-both-sets form): an S1 cloud of 21 000 atoms,
    the smallest size whose single call reads the narrow record, all candidates and contacts only.  6bft itself (8 k atoms) and a pack of it run
    kernels that keep the wide record; the same groups and the contacts-only list are checked on them against the oracle all the same."""
    path = str(synth.DATA / "6bft.pdb")
    prod, orc = aa.load_model(path), ob.Structure.load(path)
    for groups in ("A,B/C,G", "/"):
        want = orc.atomic_contacts(groups, 0.1, 6.5)
        want = want[want["kind"] != 0]
        view = prod.view(groups)
        packed = aa.atomic_contacts_batch([ctx], [view, view], aa.default_params(contacts_only=True))
        for k in range(2):
            assert_same_as_oracle(packed[k], want, f"6bft {groups} contacts only, pack member {k}")
    rec = synth.gen_s1(21000)
    chains = sorted(set(rec["chain"].tolist()))
    groups = ",".join(c.decode() for c in chains[:9]) + "/" + ",".join(c.decode() for c in chains[5:])
    soa, want = both(rec, groups)
    assert len(want) > 0
    for only in (False, True):
        got = ctx.atomic_contacts(soa, aa.default_params(contacts_only=only))
        assert ctx.rare_batches() > 0
        assert_same_as_oracle(got, want[want["kind"] != 0] if only else want, f"s1 {groups} only={only}")


@pytest.mark.gpu
def test_two_models_in_one_input(ctx):
    """Two models of 10 800 atoms each in one input: the grid has two z slabs, so a task's home cells need the atoms' model ids (read from the
    caller's array by index).  Plain kernels (no residue rule before the queue), so that pairs of one residue reach the tag test."""
    a = synth.gen_s1(10800)
    b = {k: v.copy() for k, v in a.items()}
    b["model_serial"] = b["model_serial"] + 1
    b["serial"] = b["serial"] + len(a["x"])
    b["res_id"] = b["res_id"] + a["res_id"].max() + 1
    b["x"] = b["x"] + 3.0
    rec = {k: np.concatenate([a[k], b[k]]) for k in a}
    assert len(rec["x"]) >= 20417
    soa, want = both(rec)
    assert len(np.unique(soa["model"])) == 2
    for only in (False, True):
        got = ctx.atomic_contacts(soa, aa.default_params(contacts_only=only, residue_runs=False))
        assert ctx.rare_batches() > 0
        assert_same_as_oracle(got, want[want["kind"] != 0] if only else want, f"two models, only={only}")


def test_index_bits_knob_values():
    """arp_debug_set("index_bits"): 0, a width of 1 .. 20 bits, or negative; anything wider leaves the tag fewer than 12 bits and is refused."""
    try:
        for v in (-1, 1, 15, 20, 0):
            aa.debug_set("index_bits", v)
        with pytest.raises(aa.ArpeggiaError):
            aa.debug_set("index_bits", 21)
    finally:
        aa.debug_set("index_bits", 0)


def test_tag_test_never_rejects():
    """The proof next to exact_finish_e's tag test, restated on integers: whenever (tag b - tag a + 1) mod 2^T > 2 the two atoms are not of one chain
    with ordinals at most 1 apart -- for every tag width of the record and for ordinals and chain ranks in and out of the residue word's range."""
    rng = np.random.default_rng(11)
    for ib in (1, 12, 15, 20):
        T = 32 - ib
        n = 200000
        cr = rng.integers(0, 4, n, dtype=np.uint64) * rng.choice(np.array([1, 1 << 11, (1 << 12) - 1], dtype=np.uint64), n)
        ro_a = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        gap = rng.choice(np.array([0, 1, 2, 3, (1 << T) - 2, (1 << T) - 1, 1 << T, (1 << T) + 1, (1 << T) + 2, 1 << 20], dtype=np.uint64), n)
        ro_b = (ro_a + gap * rng.choice(np.array([1, (1 << 32) - 1], dtype=np.uint64), n)) & np.uint64(0xFFFFFFFF)  # (+ gap or - gap, mod 2^32)
        cr_b = np.where(rng.random(n) < 0.7, cr, (cr + np.uint64(1)) & np.uint64(0xFFFFFFFF))
        tag = lambda c, o: (((c << np.uint64(20)) + o) & np.uint64(0xFFFFFFFF)) & np.uint64((1 << T) - 1)
        proved = ((tag(cr_b, ro_b) - tag(cr, ro_a) + np.uint64(1)) & np.uint64((1 << T) - 1)) > 2
        rejected = (cr == cr_b) & (((ro_b - ro_a + np.uint64(1)) & np.uint64(0xFFFFFFFF)) <= 2)  # complex.rs:108-113 as the kernels state it
        assert not np.any(proved & rejected)
        assert np.any(proved) and np.any(rejected)
