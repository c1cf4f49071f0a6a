"""Inputs and thresholds shared by test_block_loops_cpu.py and test_block_loops_gpu.py.

The level kernels of the bit-parallel solver are grid-stride loops over tiles of TILE[W] vertices.
With the tuning key max_grid = g one block runs ceil(items / (g * TILE[W])) tiles; the tests need
TILES_MIN of them, so the inputs below are chosen by need(W, g) = TILES_MIN * g * TILE[W]."""
import numpy as np

# Lay<W>::TILE (csrc/src/kernels/bitpar/common.hpp): vertices per block iteration
TILE = {1: 256, 2: 256, 4: 128, 8: 64, 16: 32}
GROUPS = {1: 64, 2: 128, 4: 256, 8: 512, 16: 1024}  # query groups that take W words
WORDS = (1, 2, 4, 8, 16)
MAX_GRIDS = (1, 3)
SOURCES = 8  # per group

# Tiles one lane must run: 2^7 + 1, one more than a spill period of the largest register counter,
# GroupCounts<W, D = 7, ...> of k_bu_full at 16 words (csrc/src/kernels/bitpar/pull_full.hpp;
# every other GroupCounts<...> and BitCounter<VW, D> has D = 5 or 6). add() spills after
# 2^D - 1 tiles, so a lane that runs 129 has spilled mid-loop and added again after it. Whoever
# raises D raises this.
TILES_MIN = 129


def need(W, g):
    """list entries with which a kernel at max_grid = g runs TILES_MIN tiles per lane"""
    return TILES_MIN * g * TILE[W]


# ---- graphs, by need(W, g); the per-level counts that make them large enough are asserted in
# test_block_loops_cpu.py
UNIFORM = {"U60": (60000, 600000, 1), "U120": (120000, 1200000, 1)}   # mean degree 20
# mean degree 6.7 <= 8, max degree <= 64: the graphs whose push levels run as device-driven
# batches of one-kernel levels (BitparSolver::fused_batches)
SPARSE = {"S60": (60000, 200000, 1), "S120": (120000, 400000, 1)}
RMAT_SEED = 1


def uniform_for(W, g):
    return "U60" if need(W, g) <= TILES_MIN * 256 else "U120"


def sparse_for(W, g):
    return "S60" if need(W, g) <= TILES_MIN * 256 else "S120"


def rmat_scale_for(W, g):
    """the smallest scale whose vertices of degree >= 4 (the wide list of the wide_degree = 4
    runs, the shortest list a case relies on) number need(W, g). RMAT (edge factor 16, seed 1)
    has 15541 / 29263 / 55415 / 105980 of them at scale 15 / 16 / 17 / 18, so a scale serves
    block tiles g * TILE[W] of up to 96 / 192 / 384 / 768 vertices (the twin asserts each)"""
    nd = need(W, g)
    return 15 if nd <= TILES_MIN * 96 else 16 if nd <= TILES_MIN * 192 else \
        17 if nd <= TILES_MIN * 384 else 18


def make_graph(m, name):
    if name in UNIFORM:
        return m.Graph.uniform(*UNIFORM[name])
    if name in SPARSE:
        return m.Graph.uniform(*SPARSE[name])
    assert name[0] == "R"
    return m.Graph.rmat(int(name[1:]), 16, RMAT_SEED)


LEAFY = (60000, 600000, 1)


def leafy_graph(m):
    """U60 with one leaf hung on every vertex (ids n .. 2n - 1): every core vertex is a parent of
    weight 1, the one weight class whose tiles k_leaf_weigh counts in one register counter"""
    from msbfs.models.generators import uniform_edges_np
    n = LEAFY[0]
    u, v = uniform_edges_np(*LEAFY)
    core = np.arange(n, dtype=np.int32)
    return m.Graph.from_edges(2 * n, np.concatenate([np.asarray(u, np.int32), core]),
                              np.concatenate([np.asarray(v, np.int32), core + n]))


# A tree of fan-out 60, 60 and TREE[name]: root 0, layers 1 .. 60 and 61 .. 3660, then the last
# layer, children of one vertex at consecutive ids. Every group that holds the root reaches the
# whole last layer at level 3, every group that holds a layer-1 vertex most of it at level 4: one
# counter bit set in every tile of a long run, which is what it takes to carry a register counter
# to its last value (a bit that is set in two tiles out of three, as on the random graphs, never
# does). Max degree 61 and mean degree 2: push levels run as device-driven batches too.
TREE = {"T36": 10, "T101": 28}
TREE_INNER = 1 + 60 + 3600


def tree_for(W, g):
    return "T36" if need(W, g) <= TILES_MIN * 256 else "T101"


def tree_graph(m, name):
    last = TREE[name]
    n = TREE_INNER + 3600 * last
    v = np.arange(1, n, dtype=np.int64)
    par = np.where(v <= 60, 0, np.where(v < TREE_INNER, 1 + (v - 61) // 60,
                                        61 + (v - TREE_INNER) // last))
    return m.Graph.from_edges(n, par.astype(np.int32), v.astype(np.int32))


def tree_queries(m, name, K):
    """the root; one layer-1 vertex; 8 random vertices; the root and a random vertex; and so on"""
    n = TREE_INNER + 3600 * TREE[name]
    rng = np.random.default_rng(5)
    groups = []
    for k in range(K):
        groups.append([[0], [1 + (k // 4) % 60], [int(x) for x in rng.integers(0, n, SOURCES)],
                       [0, int(rng.integers(0, n))]][k % 4])
    return m.QuerySet.from_groups(groups)


# ---- the prefix level and the LDS-hub pull (kinds 'p', 't', 'h'): the planner takes them from
# its vertex count n, isolated ids included (pull_plan.hpp: hub_big_graph, hub_lds), so a uniform
# graph whose ids are padded with isolated vertices up to PAD_N runs them on short lists.
PAD_N = (1 << 22) + 1  # hub_big_graph(n): n > kHubBig * 32 * 4 = 2^22
# ... and, for the small LDS hub bitmap (NarrowHub, not NarrowHubBig; no prefix level there):
# kHubW * 32 * 4 = 1835008 < n <= 2^22
PAD_HUB = 1 << 21
PADDED = {"P60": (60000, 600000, 1), "P120": (120000, 1200000, 1), "P420": (420000, 4200000, 1)}
# vertices per block iteration of these k_bu_narrow variants: (BT / 64) * VPW with BT = 768
# threads for the prefix pull at one word, else 1024 (pfx_block; NarrowHub: 1024)
PFX_TILE = {1: 12 * 64, 2: 16 * 64, 4: 16 * 32, 8: 16 * 16, 16: 16 * 8}
HUB_TILE = {**PFX_TILE, 1: 16 * 64}
WIDE_DEFAULT = 32  # SolverOptions::wide_degree: the first pull level's wide list starts there


def padded_for(tile, g):
    """the smallest padded graph whose narrow list (its vertices of degree < WIDE_DEFAULT) gives
    one block of `g` TILES_MIN iterations of `tile` vertices"""
    nd = TILES_MIN * g * tile
    return "P60" if nd <= 50000 else "P120" if nd <= 100000 else "P420"


def padded_graph(m, name, pad_n=PAD_N):
    """(core, padded): the uniform graph and the same CSR with isolated ids up to pad_n"""
    core = m.Graph.uniform(*PADDED[name])
    rowptr = np.concatenate([core.rowptr, np.full(pad_n - core.n, core.rowptr[-1], np.int64)])
    return core, m.Graph(pad_n, rowptr, core.col, m=core.m)


def queries(m, n, K):
    """K groups of SOURCES sources; the first K' < K of them are the query set of K' groups (the
    generator draws group by group), so every per-level vertex count below grows with K"""
    return m.QuerySet.random(n, K, SOURCES, 7)


# the levels whose lists the GPU tests rely on, per graph family
RELIED = {"U": (3, 4), "S": (4, 5, 6), "R": (2, 3)}


def level_counts(g, D):
    """From a distance matrix D[K, n]: {level: (gained, unfinished, unfinished_core)}: the vertices
    first reached by some group at the level (they gain a bit there), the non-isolated vertices
    some group reaches at this level or later (not finished when the level starts: the pull
    level's list), and those of them with degree >= 2 (the list of a leaf-folded run)."""
    deg = np.diff(g.rowptr)
    last = D.max(axis=0)
    out = {}
    for lvl in range(1, int(D.max()) + 1):
        gained = int((D == lvl).any(axis=0).sum())
        unf = (last >= lvl) & (deg > 0)
        out[lvl] = (gained, int(unf.sum()), int((unf & (deg >= 2)).sum()))
    return out


def weight1_parents(g):
    """vertices of degree >= 2 with exactly one degree-1 neighbour: the first weight class of
    k_leaf_weigh (csrc/src/kernels/bitpar/leaf_kernels.hpp), whose tiles share one counter"""
    deg = np.diff(g.rowptr)
    leaves = np.flatnonzero(deg == 1)
    par = g.col[g.rowptr[leaves]]
    par = par[deg[par] >= 2]
    return int((np.bincount(par, minlength=g.n) == 1).sum())
