"""A designed graph and designed query groups for the first pull level (numpy / scipy only), shared
by test_prefix_level_cpu.py and test_prefix_level_gpu.py.

Level 2 of a run on a big degree-relabelled graph pulls, for every vertex, the prefix of its sorted
row (the neighbours with internal id < H) and lets the level-1 vertices with id >= H push
(bitpar/tiles.hpp, bitpar/pull_tail.hpp). boundary_graph() fixes the internal ids by degree classes
alone: exactly H vertices of degree >= 3 (the body, ids [0, H)), then the vertices of degree 2 (the
tail), then the leaves, then isolated ids up to PAD_N. A vertex's prefix length is then its number
of body neighbours, and where a level-1 vertex (a carrier) stands inside a target's prefix follows
from its degree: above 8 it sorts first, with exactly 3 last, the other prefix members having
degree 4 or 5. boundary_queries() chooses the groups once the relabelling is known (sources change
no degree), census() computes levels 1 and 2 of every group from sparse products and returns the
facts test_prefix_level_cpu.py asserts. sun_graph() is the graph on which every vertex of every
tile gains every group at level 2, so that the tiled kernel's register counters are full whenever
they spill.
"""
import types

import numpy as np

import block_loops as bl
from degree_graphs import sorted_csr

H = 458752            # kPfxH = kHubW * 32 (csrc/src/kernels/bitpar/pull_plan.hpp): the tiles' bound
BIG = 1024            # kBigPrefix = kPartialEntries (bitpar/tiles.hpp): more entries: partial tiles
ROUND = 256           # kRound = 64 * kRoundQ (bitpar/tiles.hpp): entries per round of a tile
VT = 32               # kTileVT (bitpar/tiles.hpp): vertices per tile at the most
PAD_N = (1 << 22) + 1  # hub_big_graph(n): n > kHubBig * 32 * 4 (pull_plan.hpp), as block_loops.PAD_N
TILE_WAVES = 16       # kTileBlock / 64 (bitpar/tiles.hpp): waves, i.e. tiles in flight, per block

PREFIX_LENGTHS = (0, 1, 255, 256, 257, 512, 1023, 1024, 1025, 2048, 2049, 3073)
# a carrier alone at entry 0, or alone at entry L - 1: the second round, the second and the third
# partial tile
POSITIONAL = (257, 1025, 2049)
POOL_LENGTHS = (255, 256, 512, 1023, 1024, 2048, 3073)

# Rows at the start of level 2: unit i has a source that every group of ROW_SETS[i] holds, a body
# carrier (degree 3) and a tail pusher (degree 2) next to it; their rows are exactly that set.
ROW_SETS = (
    (0,), (63,), (1, 2), (3, 4, 5), (63, 64), (0, 1023), (1021, 1022, 1023), (5, 70, 130),
    (62, 63, 64, 65), tuple(range(60, 128)), (64,), (6, 7, 8, 9), (1023,), (32, 33))
# (in this order every target of the pool keeps a carrier in the first 64 groups: the sets that
# name none lie apart, and target i is pulled through the carriers of units i and i - 1)
# groups with sources of their own
G_POS = 10     # 10 .. 21: (257, 1025, 2049) x two targets x (first entry, last entry)
G_PUSH_BIG, G_ONE, G_VMAX, G_LEAF_SRC, G_HM1, G_H = 22, 23, 24, 25, 26, 27
G_CYCLE = 28   # 28 .. 31: every fourth vertex of the tail cycle, shifted by 0 .. 3
CYCLE = 128
HI_LEAVES = 170  # leaves of a first-entry carrier: its degree, above every other prefix member's
SUB_K4 = 342     # subdivided K4 components: 4 body and 6 tail vertices each


class _Build:
    def __init__(self):
        self.n, self.us, self.vs = 0, [], []

    def new(self, k):
        a = np.arange(self.n, self.n + k, dtype=np.int64)
        self.n += k
        return a

    def one(self):
        return int(self.new(1)[0])

    def edge(self, u, v):
        u, v = np.broadcast_arrays(np.asarray(u, np.int64), np.asarray(v, np.int64))
        self.us.append(u.ravel().copy())
        self.vs.append(v.ravel().copy())

    def leaves(self, v, k):
        a = self.new(k)
        self.edge(v, a)
        return a

    def cliques(self, size, count):
        """count components K_size; returns the first vertex of the first one (consecutive ids)"""
        a = self.new(size * count).reshape(count, size)
        for i in range(size):
            for j in range(i + 1, size):
                self.edge(a[:, i], a[:, j])
        return a

    def members(self, t, k):
        """k neighbours of t of degree 4 or 5: K4s and K5s whose every vertex also joins t"""
        if k == 0:
            return
        if k < 12:
            raise ValueError("members come in cliques of 4 and 5")
        k5 = k % 4
        for size, cnt in ((5, k5), (4, (k - 5 * k5) // 4)):
            if cnt:
                self.edge(t, self.cliques(size, cnt).ravel())


PETERSEN = [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + \
    [(5 + i, 5 + (i + 2) % 5) for i in range(5)]


def boundary_graph(seed=1):
    """The design graph: a namespace with n = PAD_N, n_core (the non-isolated vertices: user ids
    [0, n_core)), the edges u, v (int32, user ids, shuffled) and roles, a dict of user ids that
    boundary_queries() reads. See the module docstring and the comments below for the gadgets."""
    b = _Build()
    roles = {}
    tgt = {L: [b.one() for _ in range(2)] for L in PREFIX_LENGTHS if L >= 255}
    body_nbrs = {t: 0 for ts in tgt.values() for t in ts}  # prefix entries given so far

    def join(c, t, times=1):
        for _ in range(times):
            b.edge(c, t)
        body_nbrs[t] += times

    # ---- positional targets: one carrier of high degree (a leaf of it is the source: entry 0)
    # and one of degree exactly 3 (behind a tail source: entry L - 1), nothing else of degree
    # 3 or above 8 in the prefix
    pos = []
    for L in POSITIONAL:
        for t in tgt[L]:
            hc = b.one()
            join(hc, t)
            hl = b.leaves(hc, HI_LEAVES)
            lc, ls = b.one(), b.one()
            join(lc, t)
            b.edge(lc, ls)
            b.leaves(lc, 1)
            b.leaves(ls, 1)                     # (a leaf hung on a tail vertex)
            pos += [int(hl[0]), ls]
    roles["pos"] = pos
    roles["hi_leaf_extra"] = hc                 # (takes one more leaf if n_core % 32 == 0)
    # ---- the row-set units over the pool of the other targets
    pool = [tgt[L][j] for L in POOL_LENGTHS for j in range(2)]
    NP = len(pool)
    assert NP == len(ROW_SETS)
    unit_src = []
    for i in range(NP):
        s, c, x = b.one(), b.one(), b.one()
        b.edge(s, [c, x])
        b.leaves(s, 1)
        # unit 0: a duplicate edge between carrier and target
        join(c, pool[i], 2 if i == 0 else 1)
        if i:
            join(c, pool[(i + 1) % NP])
        # even units push to the target their carrier is pulled from (one group's bit from a
        # prefix entry and from a pusher), odd ones to another (different groups from each)
        b.edge(x, pool[i] if i % 2 == 0 else pool[(i + 5) % NP])
        unit_src.append(s)
    roles["unit_src"] = unit_src
    # ---- a big vertex reached by a push alone: a pusher of a group no carrier of the target has
    s, x = b.one(), b.one()
    b.edge(s, x)
    b.leaves(s, 2)
    b.edge(x, tgt[1025][0])
    roles["push_big"] = s
    # ---- two targets of prefix length 1: tail vertices between a body carrier and a leaf
    s, c = b.one(), b.one()
    b.edge(s, c)
    b.leaves(s, 2)
    for _ in range(2):
        t = b.one()
        b.edge(c, t)
        b.leaves(t, 1)
    roles["one"] = s
    # ---- a tail pusher whose other neighbour is a leaf (leaf folding pushes to no leaf), and a
    # leaf as a source
    s, x = b.one(), b.one()
    b.edge(s, x)
    sl = b.leaves(s, 2)
    b.leaves(x, 1)
    roles["vmax"] = s
    roles["leaf_src"] = int(sl[0])
    # ---- the vertex of the highest degree (provisional id 0) has one tail neighbour: the locality
    # key then gives that one internal id H. A self-loop on it (two entries of its own prefix)
    top = tgt[3073][1]
    s, x = b.one(), b.one()
    b.edge(s, x)
    b.leaves(s, 2)
    b.edge(x, top)
    b.edge(top, top)
    body_nbrs[top] += 2
    roles["top"] = top
    # ---- members (degree 4 or 5) up to the prefix length, two leaves on every target (a level-2
    # gain that carries leaf weight), two more on the top one
    for L, ts in tgt.items():
        for t in ts:
            b.members(t, L - body_nbrs[t])
            b.leaves(t, 4 if t == top else 2)
    # ---- the tail cycle: degree 2, tail neighbours only, so prefix length 0; the only such
    # vertices of the graph, hence the last CYCLE ids of the tail
    cyc = b.new(CYCLE)
    b.edge(cyc, np.roll(cyc, -1))
    roles["cycle"] = cyc
    # ---- the rest of the tail: subdivided K4s (body vertices with three tail neighbours each)
    sub = b.new(10 * SUB_K4).reshape(SUB_K4, 10)
    k = 4
    for i in range(4):
        for j in range(i + 1, 4):
            b.edge(sub[:, i], sub[:, k])
            b.edge(sub[:, j], sub[:, k])
            k += 1
    roles["sub"] = sub[:, 0]
    # ---- the rest of the body: Petersen graphs (3-regular, girth 5: a vertex at distance 2 has
    # one path to the source), a few K4 / K5 to land on H exactly
    u = np.concatenate(b.us)
    v = np.concatenate(b.vs)
    deg = np.bincount(np.concatenate([u, v]), minlength=b.n)
    rest = H - int((deg >= 3).sum())
    k4 = k5 = 0
    while (rest - 4 * k4 - 5 * k5) % 10:
        if (rest - 4 * k4 - 5 * k5) % 2:
            k5 += 1
        else:
            k4 += 1
    if k4:
        b.cliques(4, k4)
    if k5:
        b.cliques(5, k5)
    npet = (rest - 4 * k4 - 5 * k5) // 10
    assert npet >= 1024
    pet = b.new(10 * npet).reshape(npet, 10)
    for i, j in PETERSEN:
        b.edge(pet[:, i], pet[:, j])
    roles["petersen"] = pet[:, 0]
    if b.n % 32 == 0:
        b.leaves(roles["hi_leaf_extra"], 1)
    del roles["hi_leaf_extra"]
    n_core = b.n
    u = np.concatenate(b.us)
    v = np.concatenate(b.vs)
    rng = np.random.default_rng(seed)
    p = rng.permutation(n_core)
    order = rng.permutation(len(u))
    flip = rng.integers(0, 2, len(u)).astype(bool)[order]
    uu, vv = p[u][order], p[v][order]
    uu, vv = np.where(flip, vv, uu), np.where(flip, uu, vv)
    roles = {k: (p[np.asarray(x, np.int64)] if np.ndim(x) else int(p[x])) for k, x in roles.items()}
    return types.SimpleNamespace(n=PAD_N, n_core=n_core, u=uu.astype(np.int32),
                                 v=vv.astype(np.int32), roles=roles)


def host_graphs(m, g):
    """(core, padded): the graph on its n_core non-isolated vertices (the CPU oracle runs on it:
    no group reaches an isolated id) and the same CSR with isolated ids up to g.n"""
    core = m.Graph.from_edges(g.n_core, g.u, g.v)
    rowptr = np.concatenate([core.rowptr, np.full(g.n - core.n, core.rowptr[-1], np.int64)])
    return core, m.Graph(g.n, rowptr, core.col, m=core.m)


def _alone(rowptr, col, x):
    """(s, t): a neighbour s of x and a vertex t at distance 2 from s whose only neighbour at
    distance 1 from s is x; s of the lowest degree that has one"""
    row = lambda a: col[rowptr[a]:rowptr[a + 1]]
    for s in sorted(set(int(a) for a in row(x)) - {x}, key=lambda a: rowptr[a + 1] - rowptr[a]):
        l1 = set(int(a) for a in row(s)) - {s}
        for t in row(x):
            t = int(t)
            if t != s and t not in l1 and all(int(w) == x or int(w) not in l1 for w in row(t)):
                return s, t
    raise AssertionError(f"no level-2 vertex depends on {x} alone")


def boundary_queries(m, g, o2n, K):
    """The first K of the 1024 groups of the design graph g, given its relabelling map o2n
    (degree_graphs.relabel_oracle / DeviceGraph.relabel_map). Every group but two holds one
    vertex of a Petersen component and one of a subdivided K4 of its own; on top of that come the
    groups named above ROW_SETS. Groups G_HM1 and G_H hold one neighbour of the vertices with
    internal ids H - 1 and H, found here from the map."""
    r = g.roles
    groups = [[int(r["petersen"][k]), int(r["sub"][k % SUB_K4])] for k in range(1024)]
    for i, ks in enumerate(ROW_SETS):
        for k in ks:
            groups[k].append(int(r["unit_src"][i]))
    for j, s in enumerate(r["pos"]):
        groups[G_POS + j].append(int(s))
    groups[G_PUSH_BIG].append(r["push_big"])
    groups[G_ONE].append(r["one"])
    groups[G_VMAX].append(r["vmax"])
    groups[G_LEAF_SRC].append(r["leaf_src"])
    rowptr, col = sorted_csr(g.n_core, g.u, g.v)
    o2n = np.asarray(o2n)
    n2o = np.empty(g.n_core, np.int64)
    n2o[o2n[:g.n_core]] = np.arange(g.n_core)
    groups[G_HM1] = [_alone(rowptr, col, int(n2o[H - 1]))[0]]
    groups[G_H] = [_alone(rowptr, col, int(n2o[H]))[0]]
    for j in range(4):
        groups[G_CYCLE + j] += [int(x) for x in r["cycle"][j::4]]
    return m.QuerySet.from_groups(groups[:K])


def required_row_sets(K):
    """the 1- to 4-group rows of ROW_SETS that name no group above K - 1"""
    return [frozenset(s) for s in ROW_SETS if len(s) <= 4 and max(s) < K]


def census(g, o2n, qs):
    """Levels 1 and 2 of every group of qs on the design (or any) graph g, in internal ids, from
    two sparse products, and the facts about them that the tests assert (see the keys below).
    A row is the set of groups that reached a vertex at levels 0 and 1; a carrier is a level-1
    vertex of a group with a neighbour that the group reaches at level 2."""
    import scipy.sparse as sp
    n = g.n_core
    o2n = np.asarray(o2n, np.int64)
    assert o2n[:n].max() == n - 1  # (the isolated ids come last)
    rowptr, col = sorted_csr(n, o2n[g.u], o2n[g.v])
    col = col.astype(np.int64)
    deg = np.diff(rowptr)
    rows = np.repeat(np.arange(n), deg)
    plen = np.bincount(rows[col < H], minlength=n)
    K = qs.K
    A = sp.csr_matrix((np.ones(len(col), np.int32), col, rowptr), shape=(n, n))
    A.sum_duplicates()  # (a duplicate edge, a self-loop: multiplicity 2)
    gk = np.repeat(np.arange(K), np.diff(qs.off))
    S = sp.csr_matrix((np.ones(len(gk), np.int32), (o2n[qs.ids], gk)), shape=(n, K))
    S.data[:] = 1

    def ones(M):
        M = M.tocsr().copy()
        M.eliminate_zeros()
        M.data[:] = 1
        return M

    def minus(M, X):  # 0/1 matrices: M and not X
        D = (M - M.multiply(X)).tocsr()
        D.eliminate_zeros()
        return D

    L1 = minus(ones(A @ S), S)
    seen = ones(S + L1)
    body = sp.diags((np.arange(n) < H).astype(np.int32))
    Nb = (A @ (body @ L1)).tocsr()            # level-1 entries inside the prefix, per (v, group)
    Nt = (A @ (L1 - body @ L1)).tocsr()       # ... and behind it: the pushers
    N2 = (Nb + Nt).tocsr()
    L2 = minus(ones(N2), seen)
    l2_any = L2.getnnz(axis=1) > 0
    pulled, pushed = ones(Nb.multiply(L2)), ones(Nt.multiply(L2))
    pull_only, push_only = minus(L2, pushed), minus(L2, pulled)
    both = ones(pulled.multiply(pushed))
    carr = ones(L1.multiply(ones(A @ L2)))
    out = {"n_core": n, "body": int((deg >= 3).sum()), "tail": int((deg == 2).sum()),
           "leaves": int((deg == 1).sum()),
           # the degree classes are the id ranges
           "classes_are_ranges": bool(deg[:H].min() >= 3 and (deg[H:H + int((deg == 2).sum())] == 2).all())}
    out["level2_by_plen"] = {L: int(((plen == L) & l2_any).sum()) for L in PREFIX_LENGTHS}
    z = np.flatnonzero(np.diff(np.concatenate([[0], ((plen == 0) & l2_any).astype(np.int8), [0]])))
    out["zero_run"] = int((z[1::2] - z[::2]).max()) if len(z) else 0
    # ---- rows of the carriers
    seen = seen.tocsr()
    seen.sort_indices()
    for name, lo, hi in (("body", 0, H), ("tail", H, n)):
        sets, sizes = set(), set()
        for v in np.flatnonzero(carr.getnnz(axis=1) > 0):
            if lo <= v < hi:
                ks = seen.indices[seen.indptr[v]:seen.indptr[v + 1]]
                sizes.add(min(len(ks), 65))
                if len(ks) <= 4:
                    sets.add(frozenset(int(k) for k in ks))
        out["rows_" + name] = sets
        out["row_sizes_" + name] = sizes
    # ---- (v, k) whose only level-1 entry, counted with multiplicity, is one entry of the prefix
    L1c = L1.tocsc()
    L1c.sort_indices()
    lvl1 = lambda k: L1c.indices[L1c.indptr[k]:L1c.indptr[k + 1]]
    L2 = L2.tocsr()
    L2.sort_indices()
    first, last = {}, {}
    for v in np.flatnonzero(np.isin(plen, POSITIONAL) & l2_any):
        ent = col[rowptr[v]:rowptr[v + 1]]
        for k in L2.indices[L2.indptr[v]:L2.indptr[v + 1]]:
            at = np.flatnonzero(np.isin(ent, lvl1(k)))
            if len(at) == 1 and at[0] == 0:
                first.setdefault(int(plen[v]), (int(v), int(k)))
            if len(at) == 1 and at[0] == plen[v] - 1:
                last.setdefault(int(plen[v]), (int(v), int(k)))
    out["alone_first"], out["alone_last"] = first, last
    # ---- the bound: x is at level 1 for a group one of whose level-2 vertices has no other
    # level-1 neighbour
    for name, x in (("at_H-1", H - 1), ("at_H", H)):
        hit = None
        for k in L1.indices[L1.indptr[x]:L1.indptr[x + 1]]:
            for w in set(int(a) for a in col[rowptr[x]:rowptr[x + 1]]):
                if L2[w, k] and N2[w, k] == A[w, x]:
                    hit = (int(k), w)
        out[name] = hit
    # ---- pushed, pulled, both
    po = push_only.tocoo()
    out["push_only_plen"] = set(int(x) for x in plen[po.row])
    out["same_group_both"] = int(both.nnz)
    out["other_groups"] = int(((pull_only.getnnz(axis=1) > 0) & (push_only.getnnz(axis=1) > 0)).sum())
    # ---- leaves
    leaf_nbr = np.bincount(rows[deg[col] == 1], minlength=n) > 0
    l1_any = L1.getnnz(axis=1) > 0
    pushes = l1_any & (np.arange(n) >= H) & (deg == 2)
    out["pusher_with_leaf"] = int((pushes & leaf_nbr).sum())
    out["level2_body_with_leaf"] = int((l2_any & (np.arange(n) < H) & leaf_nbr).sum())
    out["leaf_sources"] = int((deg[o2n[qs.ids]] == 1).sum())
    out["level1"], out["level2"] = int(l1_any.sum()), int(l2_any.sum())
    out["pushers"] = int((pushes & (carr.getnnz(axis=1) > 0)).sum())
    return out


# ---- the sun: a hub next to every body vertex; 1024 handles of degree 2 between the hub and a leaf
SUN_HANDLES = 1024


def sun_need(g):
    """body vertices with which every wave of k_pfx_tiles at max_grid = g runs TILES_MIN tiles,
    each with one epilogue pass at the least: g blocks of TILE_WAVES waves, VT vertices a tile"""
    return bl.TILES_MIN * TILE_WAVES * g * VT


SUN_BODY = sun_need(max(bl.MAX_GRIDS))


def sun_graph(nbody=SUN_BODY):
    """(n, n_core, u, v): hub 0, body 1 .. nbody in a ring (degree 3 with the hub), handles
    nbody + 1 .. nbody + 1024 (hub and a leaf each), the leaves, isolated ids up to PAD_N.
    Group k = [handle k]: level 1 is the hub, with every group's bit (a dense row, a big vertex);
    at level 2 every body vertex and every other handle gains every group."""
    body = np.arange(1, nbody + 1, dtype=np.int64)
    hand = nbody + 1 + np.arange(SUN_HANDLES, dtype=np.int64)
    leaf = hand + SUN_HANDLES
    u = np.concatenate([np.zeros(nbody, np.int64), body, np.zeros(SUN_HANDLES, np.int64), hand])
    v = np.concatenate([body, np.roll(body, -1), hand, leaf])
    n_core = int(leaf[-1]) + 1
    return types.SimpleNamespace(n=PAD_N, n_core=n_core, nbody=nbody, u=u.astype(np.int32),
                                 v=v.astype(np.int32), handles=hand)


def sun_queries(m, g, K):
    return m.QuerySet.from_groups([[int(h)] for h in g.handles[:K]])
