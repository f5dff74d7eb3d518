"""The look-back cell scan (scan.inl k_scan_single) and the fix-up's copy (pairs.inl k_fixup) through the product, whole pair lists against the oracle.

(a) arp_debug_set("scan_kernel", 1 / 2) sends any input through k_scan_single on 256 / 1 024 blocks.  An S2 cloud of 20 417 atoms has about 6 000
    cells -- a few words per block on 256 blocks, most blocks of the 1 024 empty; the same cloud with its coordinates scaled by 6 has 216 times the
    volume, so the sizing coarsens the edge twice to get under the cell cap of its workspace (8 n + 64 K cells) and ends at about 135 000 cells.
    Even that is some 530 cells per block: a chunk of several register tiles (scan_unit_tile_cells = 4 096 cells) on 256 blocks needs more than
    2^20 cells, which the cap allows from about 125 000 atoms on, so a 140 000-atom cloud scaled by 6 is the case that reads its chunks twice
    (its cell count is asserted from the tests' restatement of the sizing, trajectory_shapes.grid_sizing).  tests/test_scan_unit_gpu.py holds
    the kernel's own edges.
(b) The chunked emit route with its fix-up: fresh contexts, first call (the memo of a second call would choose the staged hole-free kernels), 2 048-
    and 4 096-record chunks.  A buffer of exactly P records suffices (the tail lives partly in the engine's scratch block until the holes are
    closed), one more changes nothing, one less reports P and writes nothing behind the buffer.
(c) Plain regression cases for code this file's change left as it was, the grid sizing folded into k_cellid (grid.inl setup_block): the
    contacts-only call and a negative cutoff on the cloud and on 6bft between two chain groups, and a pack of three structures, whose sizing is
    k_setup's.  (A shorter chain of loads and barriers around the sizing was built and measured no gain -- profiles/r26_small_kernels.md -- so it
    is not in the product; the cases stay for whoever tries again.)
"""
import numpy as np
import pytest

import arpeggia_amd as aa
import oracle_binding as ob
import synth
import trajectory_shapes as ts
from arpeggia_amd import _lib
from oracle_lists import assert_same_as_oracle, both

pytestmark = pytest.mark.gpu


def scaled(rec: dict, f: float) -> dict:
    return dict(rec, x=rec["x"] * f, y=rec["y"] * f, z=rec["z"] * f)


@pytest.fixture(scope="module")
def clouds():
    """{name: (soa, oracle list)}, computed once."""
    rec = synth.gen_s2(20417)
    return {"s2 20417": both(rec), "s2 20417 x 6": both(scaled(rec, 6.0))}


@pytest.mark.parametrize("knob", [1, 2])
@pytest.mark.parametrize("name", ["s2 20417", "s2 20417 x 6"])
def test_look_back_scan_on_small_inputs(clouds, name, knob):
    soa, want = clouds[name]
    aa.debug_set("scan_kernel", knob)
    try:
        ctx = aa.Context(0)
        for det in (False, True):
            assert_same_as_oracle(ctx.atomic_contacts(soa, aa.default_params(deterministic=det)), want, f"{name}, scan_kernel {knob}, ordered={det}")
    finally:
        aa.debug_set("scan_kernel", 0)


def test_look_back_scan_over_several_tiles():
    n, tile = 140000, 4096  # (scan.inl kScanTileCells; tests/test_scan_unit_gpu.py reads it from the kernel's own library)
    rec = scaled(synth.gen_s2(n), 6.0)
    # the grid a fresh context sizes for this cloud: more cells than 256 one-tile chunks hold, so every block's chunk spans two tiles
    g = ts.grid_sizing(ts.frame_extents(np.stack([rec["x"], rec["y"], rec["z"]], 1)[None])[0], 1, n, 6.5)
    cells = g["nx"] * g["ny"] * g["nzt"]
    assert g["steps"] > 0 and 256 * tile < cells <= g["cap"], g
    soa, want = both(rec)
    aa.debug_set("scan_kernel", 1)
    try:
        ctx = aa.Context(0)
        for det in (False, True):
            assert_same_as_oracle(ctx.atomic_contacts(soa, aa.default_params(deterministic=det)), want, f"s2 140000 x 6, scan_kernel 1, ordered={det}")
    finally:
        aa.debug_set("scan_kernel", 0)


def test_scan_kernel_knob_values():
    for v in (-1, 3):
        with pytest.raises(aa.ArpeggiaError):
            aa.debug_set("scan_kernel", v)
    aa.debug_set("scan_kernel", 0)


def test_grid_sizing_inputs_on_the_cloud(clouds):
    """(c) What the folded grid sizing reads of the parameter block (grid.inl setup_block): the contacts-only flag with the three bound tables
    behind it, and the cutoff's sign (only its square counts: a negative cutoff searches the same sphere)."""
    soa, want = clouds["s2 20417"]
    ctx = aa.Context(0)
    assert_same_as_oracle(ctx.atomic_contacts(soa, aa.default_params(contacts_only=True)), want[want["kind"] != 0], "s2 20417, contacts only")
    assert_same_as_oracle(ctx.atomic_contacts(soa, aa.default_params(0.1, -6.5)), want, "s2 20417, cutoff -6.5")
    assert_same_as_oracle(ctx.atomic_contacts(soa, aa.default_params(0.1, -6.5, contacts_only=True)), want[want["kind"] != 0], "s2 20417, cutoff -6.5, contacts only")


@pytest.mark.parametrize("groups", ["H,L/C", "A,B/C,G"])
def test_grid_sizing_inputs_on_6bft_chain_groups(groups):
    """(c) The same on 6bft between two chain groups (k_cellid<2>: every block reads all the atoms; atoms outside both groups are present)."""
    path = str(synth.DATA / "6bft.pdb")
    prod, orc = aa.load_model(path), ob.Structure.load(path)
    want = orc.atomic_contacts(groups, 0.1, 6.5)
    assert len(want) > 0
    ctx = aa.Context(0)
    view = prod.view(groups)
    assert_same_as_oracle(ctx.atomic_contacts(view, aa.default_params(contacts_only=True)), want[want["kind"] != 0], f"6bft {groups}, contacts only")
    assert_same_as_oracle(ctx.atomic_contacts(view, aa.default_params(0.1, -6.5)), want, f"6bft {groups}, cutoff -6.5")


def test_grid_sizing_of_a_three_member_pack():
    """(c) k_setup shares setup_block with k_cellid: three structures packed into shared launches (one model each of the pack), all candidates and
    contacts only, each member against the oracle."""
    recs = [synth.gen_s1(1500 + 700 * k, seed=300 + k) for k in range(3)]
    pairs = [both(r) for r in recs]
    ctx = aa.Context(0)
    for only in (False, True):
        got = aa.atomic_contacts_batch([ctx], [soa for soa, _ in pairs], aa.default_params(contacts_only=only))
        for k, (_, want) in enumerate(pairs):
            assert_same_as_oracle(got[k], want[want["kind"] != 0] if only else want, f"pack member {k}, contacts only={only}")


@pytest.mark.parametrize("n", [20417, 40000, 140000])
def test_fixup_at_the_buffer_edge(n):
    torch = pytest.importorskip("torch")
    soa, want = both(synth.gen_s2(n))
    P = len(want)
    assert P > 4096
    dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in soa.items()}
    keep = []
    atoms = aa.atoms_from_arrays(dev, location=_lib.ARP_MEM_DEVICE, keep=keep)
    prm = aa.default_params()
    guard = 64
    for cap in (P, P + 1, P - 1):
        ctx = aa.Context(0, stream=torch.cuda.current_stream().cuda_stream)  # a fresh context: its first call takes the chunked route
        ctx.profile(True)
        out = torch.full((cap + guard, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ctx.enqueue(atoms, prm, out.data_ptr(), cap)
        what = f"s2 {n} atoms, capacity P{cap - P:+d}"
        if cap >= P:
            assert ctx.result() == P, what
            assert_same_as_oracle(out[:P].cpu().numpy().view(aa.PAIR_DTYPE).reshape(-1), want, what)
        else:
            with pytest.raises(aa.ArpeggiaError) as e:
                ctx.result()
            assert e.value.status == _lib.ARP_ERR_CAPACITY and str(P) in str(e.value), what
        assert "pairs_fixup" in ctx.profile_read(), f"{what}: not the chunked route"
        assert bool((out[cap:] == 0x5A5A5A5A).all()), f"{what}: written behind the buffer"
