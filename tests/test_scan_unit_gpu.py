"""The look-back cell scan k_scan_single (arpeggia_amd/csrc/scan.inl) alone, on arrays of this test's making: tests/scan_unit/scan_unit.hip includes
scan.inl and launches the kernel on 256 or 1 024 blocks with the published chunk totals zeroed first, as the grid sizing does in the product.

A block's chunk is ceil(n / blocks) cells rounded up to four, read and written as 16-byte words in tiles of `tile` cells (scan_unit_tile_cells: 256
threads x kScanTile words); a chunk of one tile stays in registers across the look-back, a longer one is read twice.  The sizes below sit on the edges
of that: nothing, less than a word, a word and one more; fewer cells than blocks and threads; blocks x tile - 1 / + 0 (the last one-tile size: every
lane of every block loaded) / + 1 (the first two-tile size, whose second tile is one word) and blocks x tile x 3 + 2 (four tiles, a ragged end).

Checked against numpy: out[0..n] is the exclusive cumulative sum with the total in out[n], in[0..n) is cleared, and the eight sentinel words behind
each array are untouched.  (`in` may be READ up to the end of the 16-byte word that holds cell n - 1 -- the sentinels are there to be read.)"""
import ctypes as C

import numpy as np
import pytest

from arpeggia_amd import build

pytestmark = pytest.mark.gpu

SENTINEL_IN, SENTINEL_OUT, PAD = 0xA5A5A5A5, 0x5A5A5A5A, 8


@pytest.fixture(scope="module")
def lib():
    so = build.build_scan_unit_library()
    lib = C.CDLL(str(so))
    lib.scan_unit_tile_cells.restype = C.c_uint32
    lib.scan_unit_run.restype = C.c_int
    lib.scan_unit_run.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    return lib


def sizes(blocks: int, tile: int) -> list:
    return [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, blocks * tile - 1, blocks * tile, blocks * tile + 1, blocks * tile * 3 + 2]


def counts(kind: str, n: int, rng) -> np.ndarray:
    if kind == "random":
        return rng.integers(0, 8, size=n, dtype=np.uint32)
    v = np.zeros(n, dtype=np.uint32)
    if kind == "one_large" and n:  # the total stays below 2^32: one count of 2^32 - 2^16 and, where there is room, a 3 behind the first word
        v[(2 * n) // 3] = 0xFFFF0000
        if n > 7:
            v[5] = 3
    return v


@pytest.mark.parametrize("kind", ["random", "zeros", "one_large"])
@pytest.mark.parametrize("blocks", [256, 1024])
def test_scan_against_numpy(lib, blocks, kind):
    tile = int(lib.scan_unit_tile_cells())
    assert tile % 1024 == 0 and tile >= 1024
    rng = np.random.default_rng(1000 * blocks + len(kind))
    for n in sizes(blocks, tile):
        v = counts(kind, n, rng)
        want = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(v, dtype=np.uint64, out=want[1:])
        assert int(want[n]) < 2**32
        a = np.concatenate([v, np.full(PAD, SENTINEL_IN, dtype=np.uint32)])
        out = np.concatenate([np.full(n + 1, 0xDEADBEEF, dtype=np.uint32), np.full(PAD, SENTINEL_OUT, dtype=np.uint32)])
        assert lib.scan_unit_run(blocks, n, a.ctypes.data, len(a), out.ctypes.data, len(out)) == 0, f"{blocks} blocks, n = {n}: HIP error"
        what = f"{blocks} blocks, {kind}, n = {n}"
        assert np.array_equal(out[: n + 1], want.astype(np.uint32)), f"{what}: first difference at cell {int(np.flatnonzero(out[: n + 1] != want.astype(np.uint32))[0])}"
        assert not a[:n].any(), f"{what}: the input is not cleared at cell {int(np.flatnonzero(a[:n])[0])}"
        assert (a[n:] == SENTINEL_IN).all(), f"{what}: written behind the input"
        assert (out[n + 1:] == SENTINEL_OUT).all(), f"{what}: written behind the output"
