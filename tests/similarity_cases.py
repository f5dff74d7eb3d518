"""Cases and references for contact similarity between frames and contact co-occurrence between rows (arp_contact_similarity, arp_bit_gram:
similarity.inl + the host half in table_ens.cpp).  No product imports: tests/test_similarity_host.py checks arp_bit_gram_host and every case's reach on
the CPU, tests/test_similarity_gpu.py runs the cases on the device.

A bitmap is the timeline bitmap: bool masks [R, F], packed by timeline_cases.pack into <u4 [R, ceil(F / 32)], frame f = bit f & 31 of word f >> 5.
  axis "frames"  the sets are the columns: S_f = { r : masks[r, f] }, M = F
  axis "rows"    the sets are the rows:    T_r = { f : masks[r, f] }, M = R

Reference: plain numpy.  sets.astype(int64) @ sets.T is the intersection matrix, its diagonal the sizes; Tanimoto = f32(f64(inter) / f64(size_a + size_b
- inter)), 1.0 where the union is empty.  One IEEE f64 divide and one rounding to f32: the device's bits are compared for equality.

The kernels' constants (similarity.inl), which the shapes below straddle:
  TILE   = 64  output tile edge of k_bit_gram (kSimTile): one workgroup per tile of the upper triangle, the mirror tile written by the same workgroup
  CHUNK  = 32  words of K that go through LDS per step (kSimChunk)
  REG    = 4   register tile edge (kSimReg): lane (tx, ty) owns outputs (ty + 16 i, tx + 16 j)
  TTILE  = 32  rows x frames of one k_bit_transpose tile; a block takes TBLOCK = 8 neighbouring words of the same 32 rows
"""
from __future__ import annotations

import functools

import numpy as np

import freq_edge_cases as fe
import timeline_cases as tc

TILE, CHUNK, REG, TTILE, TBLOCK = 64, 32, 4, 32, 8
AXES = ("frames", "rows")
METRICS = ("tanimoto", "count")
KEY = {"tanimoto": "similarity", "count": "intersection"}


def sets_of(masks: np.ndarray, axis: str) -> np.ndarray:
    masks = np.asarray(masks, bool)
    return masks.T if axis == "frames" else masks


def reference(masks: np.ndarray, axis: str) -> dict:
    """{"intersection": u4 [M, M], "similarity": f4 [M, M], "sizes": u4 [M]} of a bool [R, F] bitmap."""
    sets = sets_of(masks, axis).astype(np.int64)
    inter = sets @ sets.T
    sizes = sets.sum(1)
    union = sizes[:, None] + sizes[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        tani = np.atleast_2d(inter.astype(np.float64) / union.astype(np.float64)).astype(np.float32)
    tani[union == 0] = np.float32(1.0)
    return {"intersection": inter.astype("<u4"), "similarity": np.ascontiguousarray(tani, "<f4"), "sizes": sizes.astype("<u4")}


def assert_matrix(got, got_sizes, masks, axis: str, metric: str, what="", want: dict | None = None):
    """Byte equality of the matrix and the sizes with the numpy reference (want: reference(masks, axis) when the caller already has it)."""
    want = reference(masks, axis) if want is None else want
    key = KEY[metric]
    assert got.dtype == want[key].dtype and got.shape == want[key].shape, (what, got.dtype, got.shape, want[key].shape)
    if got.tobytes() != want[key].tobytes():
        bad = np.argwhere(got.view(np.uint32) != want[key].view(np.uint32))
        raise AssertionError(f"{what} {axis} {metric}: {len(bad)} elements differ, first {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[key][tuple(bad[0])]!r}")
    assert got_sizes.dtype == np.dtype("<u4") and np.array_equal(got_sizes, want["sizes"]), (what, "sizes")


# ---- bitmaps for arp_bit_gram_host / arp_bit_gram -------------------------------------------------------------------------------------------------
def pattern(kind: str, R: int, F: int, seed: int = 0) -> np.ndarray:
    r, f = np.arange(R)[:, None], np.arange(F)[None, :]
    if kind == "ones":
        return np.ones((R, F), bool)
    if kind == "zeros":
        return np.zeros((R, F), bool)
    if kind == "checker":
        return (r + f) % 2 == 0
    if kind == "identical":  # every row the same set
        return np.broadcast_to(np.random.default_rng(seed).random((1, F)) < 0.5, (R, F)).copy()
    if kind == "disjoint":   # row r owns the frames f % R == r
        return f % R == r
    if kind == "one_bit":    # a single set bit, in the last valid position
        m = np.zeros((R, F), bool)
        m[R - 1, F - 1] = True
        return m
    if kind == "staircase":  # row k has its first k bits set: (a, b) and (b, a) tiles differ unless the mirror transposes
        return f < r
    if kind.startswith("random"):
        return np.random.default_rng(seed).random((R, F)) < float(kind[6:])
    raise ValueError(kind)


PATTERNS = ["ones", "zeros", "identical", "disjoint", "one_bit", "random0.01", "random0.5", "random0.99"]
HOST_BITS = [1, 31, 32, 33, 64, 65, 1023, 1024, 1025, 4097]
HOST_ROWS = [1, 2, 31, 32, 33, 65]

# k_bit_gram through axis "rows" (no transpose): M = rows, K = ceil(n_bits / 32) words
GRAM_M = [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 5]
GRAM_K = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
GRAM_TAIL = 13  # bits missing from the last word of the partial variant


def gram_bits(K: int) -> tuple:
    """(n_bits with a full last word, n_bits with a partial one) for K words."""
    return 32 * K, 32 * K - GRAM_TAIL


# k_bit_transpose through axis "frames": R rows x F frames -> M = F, K = ceil(R / 32)
TRANSPOSE_R = [1, 31, 32, 33, 63, 64, 65, 100]
TRANSPOSE_F = [1, 31, 32, 33, 65, 1025]
EDGE_PATTERNS = ["ones", "zeros", "checker", "one_bit"]
EDGE_SHAPES = [(1, 1), (TILE + 1, 32 * CHUNK + 1), (2 * TILE + 1, 33), (33, 2 * TILE + 1), (100, 1025)]
MIRROR_SHAPE = (2 * TILE + 2, 2 * TILE + 2)  # staircase: three tiles per edge, both axes


def dirty(words: np.ndarray, n_bits: int) -> np.ndarray:
    """The same bitmap with every bit past n_bits set in each row's last word."""
    out = words.copy()
    if n_bits % 32:
        out[:, -1] |= np.uint32((0xFFFFFFFF << (n_bits % 32)) & 0xFFFFFFFF)
    return out


def check_bitmap_reach():
    """The shapes straddle the constants they are named for."""
    assert sorted(GRAM_M) == [1, 2, 63, 64, 65, 127, 128, 129, 197] and GRAM_M[-1] == 3 * TILE + 5
    assert GRAM_K == [1, 31, 32, 33, 65]
    for K in GRAM_K:
        full, part = gram_bits(K)
        assert (full + 31) // 32 == K == (part + 31) // 32 and full % 32 == 0 and part % 32 != 0
    assert {-(-K // CHUNK) for K in GRAM_K} == {1, 2, 3}  # one chunk, a chunk and a word, two chunks and a word
    assert {-(-R // TTILE) for R in TRANSPOSE_R} == {1, 2, 3, 4} and any(R % TTILE == 0 for R in TRANSPOSE_R) and any(R % TTILE for R in TRANSPOSE_R)
    words = {-(-F // 32) for F in TRANSPOSE_F}
    assert 1 in words and max(words) > 4 * TBLOCK and any(W % TBLOCK for W in words)  # more than one block of words, a partly filled block
    assert any(F > TILE for F in TRANSPOSE_F) and any(F > 3 * TILE for F in TRANSPOSE_F)
    R, F = MIRROR_SHAPE
    st = pattern("staircase", R, F)
    for axis in AXES:
        g = reference(st, axis)["intersection"].astype(np.int64)
        assert np.array_equal(g, g.T) and -(-g.shape[0] // TILE) == 3
        a, b = g[:TILE, TILE:2 * TILE], g[TILE:2 * TILE, :TILE]
        assert not np.array_equal(a, b) and np.array_equal(a, b.T)  # tiles (0, 1) and (1, 0) differ; a mirror without the transpose is wrong
    one = pattern("one_bit", 33, 65)
    assert one.sum() == 1 and one[32, 64]


# ---- end to end: the closed-form schedules of timeline_cases ---------------------------------------------------------------------------------------
CLOSED = ["frames_1", "frames_33", "frames_2049", "rows_1", "rows_65", "rows_129", "passes_gap", "run_boundaries"]


@functools.lru_cache(maxsize=None)
def masks_of(name: str) -> np.ndarray:
    c = tc.cases()[name]
    return tc.row_masks(c.top, c.D)[1]


def no_contact_case(F: int = 40):
    """No frame has any contact: R = 0."""
    top = fe.topology(["CC", "ON"], "AB")
    return top, fe.apart(F, top.K)


def check_reach(name: str):
    """The precondition of a closed-form case: what the schedule reaches, computed from its masks."""
    tc.check_reach(name)
    m = masks_of(name)
    R, F = m.shape
    if name.startswith("frames_"):
        assert F == int(name.split("_")[1]) and R == 5
        assert {1: F == 1, 33: TILE > F > 32, 2049: F > 32 * TILE and F % TILE == 1}[F]
        sizes = m.sum(0)
        assert len(set(sizes.tolist())) >= min(F, 2)  # frames of different size
    elif name.startswith("rows_"):
        assert R == int(name.split("_")[1])
        assert {1: R == 1, 65: R == TILE + 1 and -(-R // TTILE) == 3, 129: R == 2 * TILE + 1 and -(-R // TTILE) == 5}[R]
    elif name == "passes_gap":
        empty = ~m.any(0)
        assert empty.any() and m.any(0).any()  # frames without any contact next to frames with some
        assert reference(m, "frames")["similarity"][np.ix_(empty, empty)].min() == 1.0
    elif name == "run_boundaries":
        assert F > 32 * TILE and -(-F // 32) > 2 * CHUNK and F % 32  # rows axis: K over two chunks with a partial last word
    else:
        raise AssertionError(f"no reach check for {name}")
