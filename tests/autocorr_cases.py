"""Cases and references for contact autocorrelation and survival curves across frames (arp_contact_autocorrelation, arp_bit_autocorr: autocorr.inl + the
host half in table_ens.cpp).  No product imports: tests/test_autocorr_host.py checks arp_bit_autocorr_host and every case's reach on the CPU,
tests/test_autocorr_gpu.py runs the cases on the device.

A bitmap is the timeline bitmap: bool masks [R, F], packed by timeline_cases.pack into <u4 [R, ceil(F / 32)], frame f = bit f & 31 of word f >> 5.  For lags
t = 0 .. L:
  intermittent  acf[r, t] = #{ f < F - t : m[r, f] and m[r, f + t] }                       reference: (m[:, :F - t] & m[:, t:]).sum(1), lag by lag
  continuous    acf[r, t] = #{ f < F - t : m[r, f .. f + t] all set }                      two references, asserted equal: the iterated AND
                                                                                           y_t = y_(t-1)[:, :-1] & m[:, t:], and the sum over the row's
                                                                                           maximal runs of max(0, length - t)
  half-life     the smallest t in 1 .. L with 2 acf[t] F <= acf[0] (F - t), in Python ints; none: NONE
  sums[g, t]    the sum of acf[r, t] over the rows of group g, u64

The kernels' constants (autocorr.inl), which the shapes below straddle:
  LAGS_PER_WAVE  = 64   a lane owns one lag (kAcfLagsPerWave); the half-life is the minimum over the waves of a row
  LAGS_PER_BLOCK = 256  the lag tile of one workgroup (kAcfLagsPerBlock): a row of more lags takes several workgroups
  CHUNK_WORDS    = 512  words of a row staged through LDS per step (kAcfChunkWords), the shifted operand with LAGS_PER_BLOCK / 32 words more
  ROWS_PER_BLOCK = 4    rows of one workgroup of the run lister (kAcfRowsPerBlock: a wave per row, RUN_STEP = 64 words per step with a carried run)
  RUN_CHUNK      = 1024 run lengths of a row staged through LDS per step (kAcfRunChunk)
"""
from __future__ import annotations

import functools

import numpy as np

import similarity_cases as sc
import timeline_cases as tc

LAGS_PER_WAVE, LAGS_PER_BLOCK, CHUNK_WORDS, ROWS_PER_BLOCK, RUN_CHUNK, RUN_STEP = 64, 256, 512, 4, 1024, 64
NONE = 0xFFFFFFFF
MODES = ("intermittent", "continuous")
N_INTERACTIONS = 19


# ---- references ---------------------------------------------------------------------------------------------------------------------------------
def intermittent(masks: np.ndarray, L: int) -> np.ndarray:
    m = np.asarray(masks, bool)
    R, F = m.shape
    assert 0 <= L < F
    return np.stack([(m[:, :F - t] & m[:, t:]).sum(1) for t in range(L + 1)], 1).astype("<u4").reshape(R, L + 1)


def continuous_iterated(masks: np.ndarray, L: int) -> np.ndarray:
    m = np.asarray(masks, bool)
    R, F = m.shape
    assert 0 <= L < F
    out = np.zeros((R, L + 1), "<u4")
    y = m.copy()
    for t in range(L + 1):
        if t:
            y = y[:, :-1] & m[:, t:]
        out[:, t] = y.sum(1)
    return out


def continuous_runs(masks: np.ndarray, L: int) -> np.ndarray:
    m = np.asarray(masks, bool)
    R, F = m.shape
    out = np.zeros((R, L + 1), np.int64)
    lags = np.arange(L + 1)
    for r in range(R):
        for a, b in tc._runs_of(m[r]):
            out[r] += np.maximum(0, (b - a + 1) - lags)
    return out.astype("<u4")


def continuous(masks: np.ndarray, L: int) -> np.ndarray:
    a, b = continuous_iterated(masks, L), continuous_runs(masks, L)
    assert np.array_equal(a, b)
    return a


def half_life(acf: np.ndarray, F: int) -> np.ndarray:
    """The integer rule in Python ints, row by row."""
    out = np.full(acf.shape[0], NONE, "<u4")
    for r, row in enumerate(acf.tolist()):
        for t in range(1, len(row)):
            if 2 * row[t] * F <= row[0] * (F - t):
                out[r] = t
                break
    return out


def group_sums(acf: np.ndarray, group, n_groups: int) -> np.ndarray:
    out = np.zeros((n_groups, acf.shape[1]), "<u8")
    for r, g in enumerate(np.asarray(group).tolist()):
        out[g] += acf[r].astype(np.uint64)
    return out


def reference(masks: np.ndarray, L: int, mode: str, group=None, n_groups: int = 0) -> dict:
    masks = np.asarray(masks, bool)
    acf = intermittent(masks, L) if mode == "intermittent" else continuous(masks, L)
    out = {"autocorrelation": acf, "half_life": half_life(acf, masks.shape[1])}
    if group is not None:
        out["sums"] = group_sums(acf, group, n_groups)
    return out


def assert_same(got: dict, want: dict, what="", matrix: bool = True):
    """Byte equality of the matrix (or its absence), the half-lives and, when the reference has them, the sums."""
    if matrix:
        a, b = got["autocorrelation"], want["autocorrelation"]
        assert a.dtype == np.dtype("<u4") and a.shape == b.shape, (what, a.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what}: {len(bad)} counts differ, first (row, lag) {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}")
    else:
        assert "autocorrelation" not in got, what
    h = got["half_life"]
    assert h.dtype == np.dtype("<u4") and h.shape == want["half_life"].shape, what
    if not np.array_equal(h, want["half_life"]):
        bad = np.flatnonzero(h != want["half_life"])
        raise AssertionError(f"{what}: {len(bad)} half-lives differ, first row {bad[0]}: got {h[bad[0]]}, want {want['half_life'][bad[0]]}")
    if "sums" in want:
        assert got["sums"].dtype == np.dtype("<u8") and got["sums"].tobytes() == want["sums"].tobytes(), (what, "sums")


# ---- bitmaps -------------------------------------------------------------------------------------------------------------------------------------
def pattern(kind: str, R: int, F: int, seed: int = 0) -> np.ndarray:
    f = np.arange(F)[None, :]
    if kind == "alternating":
        return np.broadcast_to(f % 2 == 0, (R, F)).copy()
    if kind == "first_bit":
        m = np.zeros((R, F), bool)
        m[:, 0] = True
        return m
    if kind == "last_bit":
        m = np.zeros((R, F), bool)
        m[:, F - 1] = True
        return m
    if kind == "word_crossing_run":  # one run over the first word boundary the row has (or as near to it as F allows)
        m = np.zeros((R, F), bool)
        a = max(0, min(28, F - 8))
        m[:, a:min(F, a + 8)] = True
        return m
    return sc.pattern(kind, R, F, seed)


PATTERNS = ["random0.01", "random0.5", "random0.99", "ones", "zeros", "alternating", "first_bit", "last_bit", "word_crossing_run"]
HOST_ROWS = [1, 2, 33, 65]
HOST_BITS = [1, 2, 31, 32, 33, 64, 65, 1025]


def host_lags(F: int) -> list:
    return sorted({L for L in (0, 1, 31, 32, 33, F - 1) if 0 <= L < F})


# lags at the lane, wave and tile edges; F = L + 1 (the last lag has a single frame pair) and F = L + 34 (a word and two bits more)
GPU_LAGS = [0, 1, 31, 32, 33, 63, 64, 65, 2 * LAGS_PER_WAVE + 1, LAGS_PER_BLOCK - 1, LAGS_PER_BLOCK, LAGS_PER_BLOCK + 1]
GPU_LAG_SLACK = [1, 34]
# frames: bit and word edges; one staging chunk less a word, exact, and a word more; two chunks and a word, with L = 70 so that the shifted operand of a
# chunk's last words lies in the next chunk
GPU_FRAMES = [1, 31, 32, 33, 65, 32 * (CHUNK_WORDS - 1), 32 * CHUNK_WORDS, 32 * CHUNK_WORDS + 1, 32 * (CHUNK_WORDS + 1), 32 * (2 * CHUNK_WORDS + 1) - 5]
CHUNK_L = 70
GPU_ROWS = [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 65, 257]
N_GROUPS = 19


def groups_of(R: int, seed: int = 0) -> np.ndarray:
    """19 groups of which 3, 7 and 18 stay empty."""
    used = np.array([g for g in range(N_GROUPS) if g not in (3, 7, 18)])
    return used[np.random.default_rng(seed).integers(0, len(used), R)].astype("<u4")


def staircase(K: int, F: int, offset: int = 27) -> np.ndarray:
    """Row k is a single run of length k that starts at a word-straddling offset: continuous counts are max(0, k - t)."""
    m = np.zeros((K, F), bool)
    for k in range(K):
        m[k, offset:offset + k] = True
    return m


def touching_runs() -> np.ndarray:
    """Two runs that reach a word boundary from each side without joining, next to the joined ones."""
    m = np.zeros((4, 100), bool)
    m[0, 25:31] = True; m[0, 32:40] = True     # bit 31 is the gap: the first run ends one short of the boundary
    m[1, 25:32] = True; m[1, 33:40] = True     # bit 32 is the gap: the second run starts one past it
    m[2, 25:40] = True                          # joined across 31 | 32
    m[3, 60:64] = True; m[3, 64:70] = True     # joined across 63 | 64, written as two pieces
    return m


def half_life_on_equality() -> tuple:
    """(masks, F, t): rows whose intermittent count at lag t sits exactly on 2 acf[t] F == acf[0] (F - t), one above and one below, no earlier lag passing.
    F = 12, t = 4: acf[0] (F - t) = 8 acf[0] and 2 acf[t] F = 24 acf[t], so acf[0] = 3 acf[4] is equality.  The rows come from a seeded search over
    random rows; check_bitmap_reach asserts what they are."""
    F, t = 12, 4
    rng = np.random.default_rng(5)
    want = {"equal": None, "above": None, "below": None}
    for _ in range(20000):
        m = rng.random(F) < 0.55
        a = [(int((m[:F - k] & m[k:]).sum())) for k in range(t + 1)]
        if a[0] == 0 or any(2 * a[k] * F <= a[0] * (F - k) for k in range(1, t)):
            continue
        lhs, rhs = 2 * a[t] * F, a[0] * (F - t)
        key = "equal" if lhs == rhs else "above" if lhs == rhs + 2 * F else "below" if lhs == rhs - 2 * F else None
        if key and want[key] is None:
            want[key] = m
        if all(v is not None for v in want.values()):
            break
    assert all(v is not None for v in want.values())
    return np.stack([want["equal"], want["above"], want["below"]]), F, t


def late_half_life(F: int = 400, period_on: int = 150) -> np.ndarray:
    """One row whose half-life lies beyond lag 63 (the first wave of the row): a single run of 150 frames, acf[t] = 150 - t in both modes, and
    2 (150 - t) 400 <= 150 (400 - t) from t = 93 on."""
    m = np.zeros((1, F), bool)
    m[0, 10:10 + period_on] = True
    return m


def check_bitmap_reach():
    """The shapes straddle the constants they are named for."""
    assert {L // LAGS_PER_WAVE for L in GPU_LAGS} >= {0, 1, 2, 3, 4} and {L // LAGS_PER_BLOCK for L in GPU_LAGS} == {0, 1}
    assert {L % 32 for L in GPU_LAGS} >= {0, 1, 31}
    words = sorted({-(-F // 32) for F in GPU_FRAMES})
    assert words == [1, 2, 3, CHUNK_WORDS - 1, CHUNK_WORDS, CHUNK_WORDS + 1, 2 * CHUNK_WORDS + 1]
    assert CHUNK_L > 64 and CHUNK_L % 32  # the shifted operand lies two words and some bits ahead: it crosses into the next chunk
    assert sorted(GPU_ROWS) == [1, 3, 4, 5, 65, 257]
    st = staircase(70, 140)
    assert (st.sum(1) == np.arange(70)).all() and st[40, 31] and st[40, 32]
    assert np.array_equal(continuous(st, 69), np.maximum(0, np.arange(70)[:, None] - np.arange(70)[None, :]).astype("<u4"))
    tr = touching_runs()
    runs = [[b - a + 1 for a, b in tc._runs_of(r)] for r in tr]
    assert runs == [[6, 8], [7, 7], [15], [10]]
    m, F, t = half_life_on_equality()
    a = intermittent(m, F - 1).astype(np.int64)
    assert 2 * a[0, t] * F == a[0, 0] * (F - t) and 2 * a[1, t] * F > a[1, 0] * (F - t) and 2 * a[2, t] * F < a[2, 0] * (F - t)
    h = half_life(a, F)
    assert h[0] == t and h[2] == t and h[1] != t
    late = late_half_life()
    h = half_life(intermittent(late, late.shape[1] - 1), late.shape[1])
    assert h[0] == 93 and LAGS_PER_WAVE < h[0] < LAGS_PER_BLOCK
    g = groups_of(100)
    assert len(set(g.tolist())) == N_GROUPS - 3 and g.max() < N_GROUPS


# ---- end to end: the closed-form schedules of timeline_cases ---------------------------------------------------------------------------------------
CLOSED = ["frames_1", "frames_33", "frames_2049", "rows_65", "rows_129", "passes_gap", "run_boundaries"]


@functools.lru_cache(maxsize=None)
def masks_of(name: str) -> np.ndarray:
    c = tc.cases()[name]
    return tc.row_masks(c.top, c.D)[1]


def codes_of(name: str) -> np.ndarray:
    c = tc.cases()[name]
    return np.array([k[2] for k in tc.row_masks(c.top, c.D)[0]], "<u4")


def check_reach(name: str):
    """The precondition of a closed-form case, computed from its masks."""
    tc.check_reach(name)
    m = masks_of(name)
    R, F = m.shape
    if name.startswith("frames_"):
        assert F == int(name.split("_")[1])
        assert {1: F == 1, 33: F == 33, 2049: F - 1 > 8 * LAGS_PER_BLOCK - 1 and -(-F // 32) < CHUNK_WORDS}[F]
        if F > 1:
            assert m.all(1).any() and (half_life(intermittent(m, F - 1), F) == NONE).any()  # an always-present row: no half-life
    elif name.startswith("rows_"):
        assert R == int(name.split("_")[1])
    elif name == "passes_gap":
        assert (~m.any(0)).any()
    elif name == "run_boundaries":
        assert F % 32 and F - 1 > 8 * LAGS_PER_BLOCK
        lens = [b - a + 1 for r in m for a, b in tc._runs_of(r)]
        assert max(lens) == F and any(a // 32 != b // 32 for r in m for a, b in tc._runs_of(r))
    else:
        raise AssertionError(f"no reach check for {name}")
