"""The emit plan (arpeggia_amd/csrc/emit_plan.h plan_emit) on the CPU: tests/emit_plan/plan_dump.cpp, a stand-alone host program that includes nothing but
that header, answers queries.  The expected plans are written out by hand for every size at which a decision changes: the thresholds' arithmetic
(wave-tasks of 64 atoms, blocks of 4 or 12 waves, index bits), not a second copy of the function."""
import itertools
import subprocess
from collections import namedtuple
from pathlib import Path

import pytest

from arpeggia_amd.build import CSRC, hipcc

SCRATCH = 2048 * 4096  # the engine's scratch block in records (pairs.inl emit_scratch_records: kMaxHoles * kChunkRecords)
Plan = namedtuple("Plan", "route waves split blocks chunk only res narrow_ib probes patch holes variant")
QUERY = dict(per_model=0, ordered=0, only=0, skip=0, res_wanted=1, narrow_ok=1, scratch=SCRATCH, emit_kernel=0, index_bits=0)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emit_plan") / "plan_dump"
    # (hipcc as a plain C++17 host compiler: no HIP header, no device pass)
    r = subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-command-line-argument", f"-I{CSRC}",
                        str(Path(__file__).resolve().parent / "emit_plan" / "plan_dump.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args, stdin=""):
        r = subprocess.run([str(exe), *args], input=stdin, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def plans(dump, queries):
    """queries: dicts of n + whatever differs from QUERY."""
    qs = [dict(QUERY, **q) for q in queries]
    text = "".join("{n} {per_model} {ordered} {only} {skip} {res_wanted} {narrow_ok} {scratch} {emit_kernel} {index_bits}\n".format(**q) for q in qs)
    out = dump(stdin=text)
    assert len(out) == len(qs)
    return [Plan(f[0], *map(int, f[1:])) for f in (line.split() for line in out)]


def plan(dump, n, **kw):
    return plans(dump, [dict(n=n, **kw)])[0]


def test_constants(dump):
    c = {k: int(v) for k, v in (line.split() for line in dump("constants"))}
    assert (c["kDirectTasks"], c["kEightTasks"], c["kSharedTasks"], c["kStageTasks"], c["kDirectBlocks"]) == (320, 160, 4608, 2048, 1536)
    assert (c["kEWaves"], c["kEBlocks"], c["kDeferBlocks"], c["kEmitBlocks"]) == (12, 512, 384, 768)
    assert (c["kChunkRecords"], c["kSmallChunkRecords"], c["kWaveStageRecords"]) == (4096, 2048, 1024)
    assert (c["kESlotBits"], c["kBigSlots"], c["kNarrowMaxBits"]) == (24, 0x5000000, 20)
    # SMALL_ROUTE and STAGE_ROUTE of tests/test_edge_rules_gpu.py, the sizes its motif sets are padded to
    assert (64 * c["kDirectTasks"], 64 * c["kStageTasks"]) == (20480, 131072)


def test_variants(dump):
    """The dispatch list: 24 different kernels, each one k_emit's static_asserts accept."""
    keys = [tuple(map(int, line.split())) for line in dump("variants")]
    assert len(keys) == 24 and len(set(keys)) == 24
    for waves, split, only, direct, res, stage, narrow in keys:
        assert waves == (4 if direct else 12) and split in ((8, 4) if direct else (4, 1))
        assert not (stage and (direct or split != 4)) and not (direct and (res or narrow)) and not (stage and narrow)


def test_table(dump):
    """Single inputs, default knobs, no memo, residue runs wanted, narrow record allowed -- unless the row says otherwise."""
    no_tail = dict(chunk=0, probes=0, patch=0, holes=0)

    def check(p, **want):
        got = {k: getattr(p, k) for k in want}
        assert got == want, p

    check(plan(dump, 0), route="Direct", waves=4, split=8, blocks=1, narrow_ib=0, res=0, **no_tail)
    check(plan(dump, 10176), route="Direct", waves=4, split=8, blocks=318, narrow_ib=0, res=0, **no_tail)
    check(plan(dump, 10177), route="Direct", waves=4, split=4, blocks=160, narrow_ib=0, res=0, **no_tail)
    check(plan(dump, 20416), route="Direct", waves=4, split=4, blocks=319, narrow_ib=0, res=0, **no_tail)
    for only in (0, 1):
        check(plan(dump, 20417, only=only), route="Chunked", waves=12, split=4, chunk=2048, blocks=107, res=1, narrow_ib=15, only=only, probes=1, patch=1 - only,
              holes=107 + (384 if only else 0))  # (k_pairs_deferred's blocks add holes of their own, k_patch_deferred's do not)
    check(plan(dump, 20417, skip=1), route="Stage", waves=12, split=4, blocks=107, res=1, narrow_ib=0, **no_tail)
    check(plan(dump, 20417, skip=1, scratch=107 * 12 * 1024), route="Stage")
    # the waves' regions do not fit the scratch block: chunked as without the memo, only the probe pass stays away
    check(plan(dump, 20417, skip=1, scratch=107 * 12 * 1024 - 1), route="Chunked", waves=12, split=4, chunk=2048, blocks=107, res=1, narrow_ib=15, probes=0, patch=1, holes=107)
    check(plan(dump, 131072, skip=1), route="Stage", split=4, blocks=512, narrow_ib=0, **no_tail)
    check(plan(dump, 131072), route="Chunked", split=4, narrow_ib=17)
    check(plan(dump, 131073, skip=1), route="Chunked", split=4, blocks=512, narrow_ib=18, probes=0, holes=512)
    check(plan(dump, 294848), route="Chunked", waves=12, split=4, chunk=2048, blocks=512, narrow_ib=19)
    check(plan(dump, 294849), route="Chunked", waves=12, split=1, chunk=4096, blocks=384, narrow_ib=19)  # 4608 tasks on 12-wave blocks
    check(plan(dump, 6144 * 64 + 1), route="Chunked", split=1, chunk=4096, blocks=512)                   # ... and the first size that fills all kEBlocks
    check(plan(dump, 1048576), route="Chunked", split=1, narrow_ib=20, res=1)
    check(plan(dump, 1048577), route="Chunked", split=1, narrow_ib=0, res=1)
    check(plan(dump, 2 ** 24 - 65), route="Chunked", waves=12, split=1, narrow_ib=0, res=1, patch=1)
    check(plan(dump, 2 ** 24 - 64), route="Gather", waves=8, blocks=768, chunk=4096, narrow_ib=0, res=0, probes=1, patch=0, holes=768 + 384)
    check(plan(dump, 0x5000000 - 1), route="Gather")
    check(plan(dump, 0x5000000), route="Ordered", res=0, narrow_ib=0, holes=0)
    check(plan(dump, 20000, per_model=1), route="Chunked", waves=12, split=4, chunk=2048, res=1, narrow_ib=0)  # packs: never Direct, Stage or narrow
    check(plan(dump, 20000, per_model=1, skip=1), route="Chunked", narrow_ib=0)
    check(plan(dump, 40000, per_model=1), route="Chunked", narrow_ib=0)
    check(plan(dump, 40000, ordered=1), res=0, narrow_ib=0)
    check(plan(dump, 40000, index_bits=-1), route="Chunked", narrow_ib=0)
    check(plan(dump, 40000, index_bits=16), route="Chunked", narrow_ib=16)
    check(plan(dump, 40000, index_bits=15), route="Chunked", narrow_ib=0)  # 15 bits do not hold index 39 999
    check(plan(dump, 40000, emit_kernel=1), route="Gather", narrow_ib=0, blocks=79, holes=79 + 384)
    check(plan(dump, 40000, narrow_ok=0), route="Chunked", narrow_ib=0, res=1)  # the table path
    check(plan(dump, 40000, res_wanted=0), route="Chunked", narrow_ib=16, res=0)


def test_sweep(dump):
    """Every size at which a decision changes, +-1, crossed with the switches: a k_emit plan has its kernel in the dispatch list, the narrow record is the
    chunked 12-wave kernels' of single inputs, the residue words are used only where the query offers them, and the hole list holds the plan's holes."""
    edges = [1, 64 * 159, 64 * 160, 64 * 319, 64 * 320, 64 * 1536, 64 * 2048, 64 * 4607, 64 * 4608, 64 * 6144, 2 ** 24 - 64, 0x5000000]
    edges += [2 ** k for k in range(14, 24)]
    sizes = sorted({max(0, e + d) for e in edges for d in (-65, -64, -63, -1, 0, 1, 2, 63, 64, 65)} | {2 ** 32 - 17})  # (the last: the largest input the engine takes)
    flags = list(itertools.product((0, 1), repeat=6))
    knobs = [(0, 0), (1, 0), (0, -1), (0, 14), (0, 17), (0, 20)]
    scratches = [SCRATCH, 107 * 12 * 1024 - 1, 0]
    qs = [dict(n=n, per_model=pm, ordered=o, only=on, skip=sk, res_wanted=rw, narrow_ok=nk, emit_kernel=ek, index_bits=ib, scratch=sc)
          for n in sizes for pm, o, on, sk, rw, nk in flags for ek, ib in knobs for sc in scratches]
    routes = set()
    for q, p in zip(qs, plans(dump, qs)):
        routes.add(p.route)
        if p.route in ("Direct", "Stage", "Chunked"):
            assert p.variant >= 0, (q, p)
            assert p.blocks >= 1 and p.blocks <= (1536 if p.route == "Direct" else 512), (q, p)
        else:
            assert p.variant == -1, (q, p)
        if p.narrow_ib:
            assert p.route == "Chunked" and p.waves == 12 and not q["per_model"] and q["narrow_ok"] and not q["ordered"], (q, p)
            assert q["n"] - 1 < 2 ** p.narrow_ib <= 2 ** 20, (q, p)
        if p.res:
            assert q["res_wanted"] and not q["ordered"] and p.route != "Direct", (q, p)
        assert p.holes <= 2048 and (p.holes == 0) == (p.route in ("Ordered", "Direct", "Stage")), (q, p)
        assert p.only == q["only"], (q, p)
    assert routes == {"Ordered", "Gather", "Direct", "Stage", "Chunked"}
