"""Cases and references for clustering the frames of an ensemble by their contacts (arp_contact_clusters, arp_bit_cluster: cluster.inl + the host half in
table_ens.cpp).  No product imports: tests/test_cluster_host.py checks arp_bit_cluster_host and every case's reach on the CPU, tests/test_cluster_gpu.py
runs the cases on the device.

A bitmap is the timeline bitmap: bool masks [R, F], packed by timeline_cases.pack.  On axis "frames" the sets are its columns (M = F), on axis "rows" its
rows (M = R), as in similarity_cases.

Reference: plain numpy.  The neighbour relation is similarity_cases.reference(masks, axis)["similarity"] >= float32(min_similarity), compared in f32; the
clusters are the loop of the header written naively -- every round recounts the alive neighbours of every alive set and takes the first maximum.

The kernels' constants (cluster.inl), which the shapes below straddle:
  TILE       = 64   tile edge of k_bit_adjacency (kSimTile): one workgroup per tile of the upper triangle, the mirror tile written by the same workgroup
  WORD       = 32   neighbour bits per word: a tile is 64 rows x 2 words
  CHUNK      = 32   words of K that go through LDS per step (kSimChunk)
  ROWS       = 64   sets per workgroup of k_cluster_round (kClusterRows), 16 per wave
  TAIL       = 256  alive words per step of k_cluster_tail
  COUNT_TILE = 4096 clusters per histogram sweep of k_cluster_counts
"""
from __future__ import annotations

import numpy as np

import similarity_cases as sc

TILE, WORD, CHUNK, ROWS, TAIL, COUNT_TILE = 64, 32, 32, 64, 256, 4096
NONE = 0xFFFFFFFF
NAN_BITS = 0x7FC00000
AXES = sc.AXES
PER_SET = ("cluster", "similarity_to_centre", "n_neighbours", "sizes")
PER_CLUSTER = ("centre", "cluster_size")


def adjacency(masks: np.ndarray, axis: str, min_similarity) -> tuple:
    """(bool [M, M] neighbour relation, the f32 similarity matrix, the sizes)."""
    ref = sc.reference(masks, axis)
    return ref["similarity"] >= np.float32(min_similarity), ref["similarity"], ref["sizes"]


def gromos(adj: np.ndarray, max_clusters: int | None = None, recount: bool = True) -> tuple:
    """(cluster [M] u4, centre [C], cluster_size [C]) of a neighbour relation.  recount False is the WRONG variant that ranks by the initial degree."""
    M = len(adj)
    a32 = adj.astype(np.float32)  # (counts below 2^24: exact)
    alive = np.ones(M, bool)
    cluster = np.full(M, NONE, "<u4")
    centre, size = [], []
    degree = adj.sum(1)
    while alive.any() and (max_clusters is None or len(centre) < max_clusters):
        n = (a32 @ alive.astype(np.float32)).astype(np.int64) if recount else degree
        c = int(np.argmax(np.where(alive, n, -1)))  # the first maximum: the smallest index among equals
        members = alive & adj[c]
        cluster[members] = len(centre)
        centre.append(c)
        size.append(int(members.sum()))
        alive &= ~members
    return cluster, np.array(centre, "<u4"), np.array(size, "<u4")


def expected(masks: np.ndarray, axis: str, min_similarity, max_clusters: int | None = None, counts: bool = True) -> dict:
    """Every output of the cluster calls for a bool [R, F] bitmap."""
    masks = np.asarray(masks, bool)
    adj, sim, sizes = adjacency(masks, axis, min_similarity)
    M = len(adj)
    cluster, centre, size = gromos(adj, max_clusters)
    to_centre = np.full(M, NAN_BITS, "<u4").view("<f4")
    got = cluster != NONE
    to_centre[got] = sim[np.arange(M)[got], centre[cluster[got]]]
    out = {"cluster": cluster, "similarity_to_centre": to_centre, "n_neighbours": adj.sum(1).astype("<u4"), "sizes": sizes, "centre": centre, "cluster_size": size,
           "n_clusters": len(centre)}
    if counts and axis == "frames":
        cc = np.zeros((masks.shape[0], len(centre)), "<u4")
        r, f = np.nonzero(masks[:, got])
        np.add.at(cc, (r, cluster[got][f]), 1)
        out["cluster_counts"] = cc
    return out


def assert_clusters(got: dict, want: dict, what=""):
    """Byte equality of every output with the reference."""
    assert got["n_clusters"] == want["n_clusters"], (what, "n_clusters", got["n_clusters"], want["n_clusters"])
    for key in PER_SET + PER_CLUSTER + (("cluster_counts",) if "cluster_counts" in want else ()):
        g, w = np.asarray(got[key]), want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
            raise AssertionError(f"{what} {key}: {len(bad)} elements differ, first {bad[0].tolist()}: got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")
    if "cluster_counts" not in want:
        assert "cluster_counts" not in got, what
    assert (np.diff(got["cluster_size"].astype(np.int64)) <= 0).all(), (what, "sizes must not increase")


def thresholds(masks: np.ndarray, axis: str) -> list:
    """0, 1, and two values the bitmap's own similarities attain (the median and the ninth decile of the pairs): few clusters, and many."""
    sim = sc.reference(masks, axis)["similarity"]
    M = len(sim)
    out = [0.0, 1.0]
    if M > 1:
        off = np.sort(sim[~np.eye(M, dtype=bool)])
        out += [float(off[len(off) // 2]), float(off[(len(off) * 9) // 10])]
    return out


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------------------
HOST_ROWS = [1, 2, 31, 32, 33, 65]
HOST_BITS = [1, 31, 32, 33, 64, 65, 1025]
DENSITIES = [0.01, 0.5, 0.99]
ROWS_M = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 197]   # word rows clustered (no transpose): adjacency-word and tile edges, three tiles with a partial last
ROWS_K = [1, 31, 32, 33, 65]                                  # words of K, each with a full and a partial last word (similarity_cases.gram_bits)
TRANSPOSE_R = [1, 31, 32, 33, 65, 100]
TRANSPOSE_F = [1, 31, 32, 33, 65, 1025]


def check_shape_reach():
    assert {-(-M // WORD) for M in ROWS_M} >= {1, 2, 3, 4, 5, 7} and {-(-M // TILE) for M in ROWS_M} == {1, 2, 3, 4}
    assert any(M % WORD == 0 for M in ROWS_M) and any(M % TILE == 0 for M in ROWS_M) and ROWS_M[-1] == 3 * TILE + 5
    assert any(M % TILE and (M % TILE) <= WORD for M in ROWS_M if M > TILE)   # a last tile whose second word does not exist
    assert {-(-K // CHUNK) for K in ROWS_K} == {1, 2, 3}
    assert max(TRANSPOSE_F) > 4 * ROWS and -(-max(TRANSPOSE_F) // WORD) > WORD  # more than one wave's stride of neighbour words


# ---- directed cases: (sets bool [M, N], min_similarity); the sets are the ROWS of the returned bitmap (axis "rows"), its transpose puts them on axis "frames" --
def graph_sets(M: int, edges: list) -> np.ndarray:
    """Sets whose Tanimoto value is positive exactly along the edges: every vertex owns one private element and one element per incident edge."""
    s = np.zeros((M, M + len(edges)), bool)
    s[np.arange(M), np.arange(M)] = True
    for k, (a, b) in enumerate(edges):
        s[a, M + k] = s[b, M + k] = True
    return s


def case_attained():
    """|A AND B| = 1, |A OR B| = 3: the value f32(1/3) is attained; a threshold equal to it passes, the next f32 above it does not."""
    sets = np.zeros((3, 5), bool)
    sets[0, [0, 1]] = sets[1, [1, 2]] = sets[2, [3, 4]] = True
    at = np.float32(1.0) / np.float32(3.0)
    above = np.nextafter(at, np.float32(2.0), dtype=np.float32)
    sim = sc.reference(sets, "rows")["similarity"]
    assert sim[0, 1] == at and sim[0, 1].tobytes() == np.float32(1 / 3).tobytes() and above > at and sim[0, 2] == 0
    assert expected(sets, "rows", at)["n_clusters"] == 2 and expected(sets, "rows", above)["n_clusters"] == 3
    return sets, at, above


def case_tie():
    """A path 0 - 1 - 2 - 3: frames 1 and 2 both have three neighbours; 1 wins and takes {0, 1, 2}; 2 would have taken {1, 2, 3}."""
    sets = np.zeros((4, 10), bool)
    for k in range(4):
        sets[k, 2 * k:2 * k + 4] = True
    thr = 0.3
    adj, _, _ = adjacency(sets, "rows", thr)
    n = adj.sum(1)
    assert n.tolist() == [2, 3, 3, 2] and not np.array_equal(adj[1], adj[2])
    cluster, centre, _ = gromos(adj)
    assert centre.tolist() == [1, 3] and cluster.tolist() == [0, 0, 0, 1]
    return sets, thr


def case_alive_counts():
    """Three neighbourhoods overlapping in a chain: c with p1 .. p6; X with p1 .. p4 and Y; Y with X and Z1 .. Z3.  c (7 neighbours) goes first and takes the
    p's.  X had 6 neighbours, the second-highest degree, but only Y is left of them: Y (5, all alive) is the next centre and takes X and the Z's.  Ranking by
    the initial degree takes X next, with Y alone, and leaves the Z's as singletons.  (Three cliques cannot show this: the frames two cliques share are
    neighbours of everybody in both, so they win the first round and take the whole of the next clique with them.)"""
    c, p, X, Y, Z = 0, list(range(1, 7)), 7, 8, [9, 10, 11]
    edges = [(c, q) for q in p] + [(X, q) for q in p[:4]] + [(X, Y)] + [(Y, z) for z in Z]
    sets = graph_sets(12, edges)
    thr = 0.01
    adj, sim, _ = adjacency(sets, "rows", thr)
    want_adj = np.eye(12, dtype=bool)
    for a, b in edges:
        want_adj[a, b] = want_adj[b, a] = True
    assert np.array_equal(adj, want_adj) and sim[adj].min() > thr
    degree = adj.sum(1)
    assert degree[c] == 7 and degree[X] == 6 and degree[Y] == 5 and sorted(degree)[-2] == degree[X]
    right, centre, _ = gromos(adj)
    wrong, wrong_centre, _ = gromos(adj, recount=False)
    alive = right != 0
    second = (adj[:, alive].sum(1))[alive]
    assert second[list(np.nonzero(alive)[0]).index(X)] == 2 != degree[X]            # the second-round count differs from the initial degree
    assert centre.tolist() == [c, Y] and wrong_centre.tolist()[:2] == [c, X] and not np.array_equal(right, wrong)
    return sets, thr


def case_identical_groups(sizes=(5, 4, 3, 2, 1), empty: int = 0):
    """Groups of identical sets, pairwise disjoint, shuffled; `empty` empty sets on top (identical to each other: one more group)."""
    rows = []
    for g, n in enumerate(sizes):
        s = np.zeros(3 * len(sizes), bool)
        s[3 * g:3 * g + 2 + (g % 2)] = True
        rows += [s] * n
    rows += [np.zeros(3 * len(sizes), bool)] * empty
    order = np.random.default_rng(5).permutation(len(rows))
    return np.array(rows)[order]


def case_distinct(M: int = 65):
    """M distinct, non-empty sets: set k holds the binary digits of k + 1."""
    sets = ((np.arange(1, M + 1)[:, None] >> np.arange(int(M).bit_length())[None, :]) & 1).astype(bool)
    assert len({bytes(s) for s in sets}) == M and sets.any(1).all()
    want = expected(sets, "rows", 1.0)
    assert want["n_clusters"] == M and want["centre"].tolist() == list(range(M)) and M > TILE
    return sets


def case_staircase():
    """similarity_cases' staircase (row k has its first k bits set: tan = min / max) at 1/2: neighbour tiles (0, 1) and (1, 0) differ, and neither is symmetric."""
    R, F = sc.MIRROR_SHAPE
    sets = sc.pattern("staircase", R, F)
    adj, _, _ = adjacency(sets, "rows", 0.5)
    a, b = adj[:TILE, TILE:2 * TILE], adj[TILE:2 * TILE, :TILE]
    assert a.any() and not a.all() and not np.array_equal(a, b) and np.array_equal(a, b.T) and not np.array_equal(a, a.T)
    return sets, 0.5


def check_directed_reach():
    case_attained(), case_tie(), case_alive_counts(), case_distinct(), case_staircase(), check_shape_reach()
    g = case_identical_groups()
    want = expected(g, "rows", 1.0)
    assert want["n_clusters"] == 5 and want["cluster_size"].tolist() == [5, 4, 3, 2, 1]
    for cap in (1, 2):
        w = expected(g, "rows", 1.0, cap)
        assert w["n_clusters"] == cap and (w["cluster"] == NONE).sum() == 15 - sum([5, 4][:cap])
        assert (w["similarity_to_centre"].view("<u4")[w["cluster"] == NONE] == NAN_BITS).all()
    e = expected(case_identical_groups(empty=2), "rows", 1.0)
    assert e["n_clusters"] == 6 and sorted(e["cluster_size"].tolist()) == [1, 2, 2, 3, 4, 5]
    for M in (33, 65):
        ones = expected(np.ones((M, 40), bool), "rows", 1.0)
        assert (ones["n_neighbours"] == M).all() and ones["n_clusters"] == 1 and M % WORD and M not in (64, 128)
