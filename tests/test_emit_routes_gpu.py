"""The emit plan's routes at their size boundaries on the device (emit_plan.h: kEightTasks, kDirectTasks): 10 176 / 10 177 atoms (159 / 160 wave-tasks:
the 4-wave hole-free kernels with the eight-way / four-way task split) and 20 416 / 20 417 atoms (319 / 320: the last 4-wave size / the first 12-wave
one: chunks, probe pass and fix-up on the first call, the scratch-staged hole-free kernels once the engine's memo says the input defers nothing).
S2 clouds: no hydrogens and no CYS pairs, so nothing is deferred and the memo is set by the first call.  The inputs are resident on the device -- the
memo names device arrays; a host input is staged afresh by every call and never gets one -- and go through the synchronous call (arp_contacts_atomic),
which feeds the profiler: `pairs_fixup` is timed exactly when the route is the chunked one.  tests/test_emit_plan_host.py holds the plans themselves."""
import numpy as np
import pytest

import arpeggia_amd as aa
import synth
from arpeggia_amd import _lib
from oracle_lists import assert_same_as_oracle, both

pytestmark = pytest.mark.gpu

CHUNKED_FROM = 20417  # 64 * (kDirectTasks - 1) + 1


@pytest.mark.parametrize("n", [10176, 10177, 20416, 20417])
def test_route_boundaries(n):
    torch = pytest.importorskip("torch")
    soa, want = both(synth.gen_s2(n))
    assert len(want) > 0
    dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in soa.items()}
    keep = []
    atoms = aa.atoms_from_arrays(dev, location=_lib.ARP_MEM_DEVICE, keep=keep)
    ctx = aa.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.profile(True)
    for call, only in enumerate((False, False, True)):
        got = ctx.atomic_contacts(atoms, aa.default_params(contacts_only=only))
        timed = ctx.profile_read()
        assert "pairs_emit" in timed, f"{n} atoms, call {call}: the call did not feed the profiler ({sorted(timed)})"
        # chunked only at 20 417 atoms, and there only before the memo is set (call 0); calls 1 and 2 run the staged kernels, all candidates and contacts only
        assert ("pairs_fixup" in timed) == (n >= CHUNKED_FROM and call == 0), f"{n} atoms, call {call}: kernels timed {sorted(timed)}"
        assert_same_as_oracle(got, want[want["kind"] != 0] if only else want, f"s2 {n} atoms, call {call}, only={only}")
