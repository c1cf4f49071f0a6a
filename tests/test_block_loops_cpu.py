"""The inputs of test_block_loops_gpu.py are large enough, shown on the inputs alone: per-level
vertex counts from the CPU oracle's distances against need(W, max_grid) = 129 tiles per lane
(block_loops.py), for every graph the GPU test picks and every level it relies on. No GPU."""
import numpy as np
import pytest

import block_loops as bl

_USES = {}  # graph name -> the largest need(W, g) among the (W, g) that pick it
for _W in bl.WORDS:
    for _g in bl.MAX_GRIDS:
        for _name in (bl.uniform_for(_W, _g), bl.sparse_for(_W, _g),
                      "R%d" % bl.rmat_scale_for(_W, _g)):
            _USES[_name] = max(_USES.get(_name, 0), bl.need(_W, _g))


def test_every_word_count_has_a_graph():
    assert set(_USES) == {"U60", "U120", "S60", "S120", "R15", "R16", "R17", "R18"}
    # one block at one or two words needs TILES_MIN * 256 list entries: the 60000-vertex graphs
    assert bl.need(1, 1) == bl.need(2, 1) == 129 * 256 == _USES["U60"] == _USES["S60"]
    assert bl.need(16, 1) == 129 * 32 and bl.need(1, 3) == 3 * 129 * 256 == _USES["U120"]


@pytest.mark.parametrize("name", sorted(_USES))
def test_levels_are_large_enough(msbfs_pkg, name):
    m = msbfs_pkg
    nd = _USES[name]
    g = bl.make_graph(m, name)
    deg = np.diff(g.rowptr)
    # 64 groups, the fewest any run uses: more groups only add vertices to every count
    qs = bl.queries(m, g.n, bl.GROUPS[1])
    assert qs == bl.queries(m, g.n, bl.GROUPS[16]).subset(range(qs.K))
    D = m.cpu_bfs(g, qs, distances=True).dist
    lc = bl.level_counts(g, D)
    print(name, "need", nd, "levels", lc)
    fam = name[0]
    for lvl in bl.RELIED[fam]:
        gained, unfinished, core = lc[lvl]
        assert gained >= nd, (name, lvl, gained, nd)          # touched list, next frontier
        assert unfinished >= nd, (name, lvl, unfinished, nd)  # the pull level's active list
        if fam == "R":
            assert core >= nd, (name, lvl, core, nd)          # ... of a leaf-folded run
            # ... and its frontiers, which hold no leaf
            assert gained - int((deg == 1).sum()) >= nd, (name, lvl, gained, nd)
    if fam == "S":
        # the push batches' graphs: k_td_fused and the vertex-parallel expansion
        assert deg.max() <= 64 and g.nnz <= 8 * g.n
    if fam == "U":
        assert deg.max() <= 64 and deg.min() > 0 and g.nnz > 8 * g.n
    if fam == "R":
        # level 2's wide list of the wide_degree = 4 runs: the unfinished vertices of degree >= 4
        last = D.max(axis=0)
        wide = int(((deg >= 4) & (last >= 2)).sum())
        assert wide >= nd, (name, wide, nd)
        assert deg.max() > 1024  # the load-balanced expansion and the later levels' chunk pulls
        # (too few for k_leaf_weigh's counters to spill mid-loop: that is the leafy graph's part)
        print(name, "wide", wide, "weight-1 parents", bl.weight1_parents(g))


def test_leafy_graph_fills_the_leaf_counters(msbfs_pkg):
    """k_leaf_weigh adds one tile of parents of one weight class per step to a BitCounter<VW, 6>:
    the leafy graph's parents all have weight 1, and there are enough of them for 2^6 + 1 tiles
    per lane at every word count and max_grid."""
    m = msbfs_pkg
    g = bl.leafy_graph(m)
    deg = np.diff(g.rowptr)
    w1 = bl.weight1_parents(g)
    print("leafy", g.n, "leaves", int((deg == 1).sum()), "weight-1 parents", w1)
    assert int((deg == 1).sum()) * 8 >= int((deg > 0).sum())  # (auto folding would fold it too)
    for W in bl.WORDS:
        for mg in bl.MAX_GRIDS:
            assert w1 >= (2 ** 6 + 1) * mg * bl.TILE[W], (W, mg, w1)
    # ... and its pull levels' lists (the unfinished vertices of degree >= 2) are as long as need()
    qs = bl.queries(m, bl.LEAFY[0], bl.GROUPS[1])
    lc = bl.level_counts(g, m.cpu_bfs(g, qs, distances=True).dist)
    print("leafy levels", lc)
    for lvl in bl.RELIED["U"]:
        assert lc[lvl][2] >= bl.need(1, 1), (lvl, lc[lvl])


@pytest.mark.parametrize("name", sorted(bl.TREE))
def test_tree_fills_whole_counters(msbfs_pkg, name):
    """The last layer is as long as need() and is reached whole, at one level, by every group
    that holds the root; nearly whole, one level later, by a group that holds a layer-1 vertex."""
    m = msbfs_pkg
    g = bl.tree_graph(m, name)
    deg = np.diff(g.rowptr)
    nd = max(bl.need(W, mg) for W in bl.WORDS for mg in bl.MAX_GRIDS if bl.tree_for(W, mg) == name)
    assert g.n - bl.TREE_INNER >= nd and deg.max() <= 64 and g.nnz <= 8 * g.n
    qs = bl.tree_queries(m, name, 8)
    D = m.cpu_bfs(g, qs, distances=True).dist
    assert (D[0, bl.TREE_INNER:] == 3).all() and (D[3, bl.TREE_INNER:] <= 3).all()
    assert int((D[1, bl.TREE_INNER:] == 4).sum()) == 59 * 60 * bl.TREE[name]
    # 2^7 tiles of 32 vertices in a row, at the least, for the widest counter
    assert 60 * bl.TREE[name] * 59 >= 128 * 3 * 32


_PADDED = {}  # padded graph name -> the largest TILES_MIN * g * tile among the cases that pick it
for _tiles in (bl.PFX_TILE, bl.HUB_TILE):
    for _W in bl.WORDS:
        for _g in bl.MAX_GRIDS:
            _name = bl.padded_for(_tiles[_W], _g)
            _PADDED[_name] = max(_PADDED.get(_name, 0), bl.TILES_MIN * _g * _tiles[_W])


@pytest.mark.parametrize("name", sorted(bl.PADDED))
def test_padded_graph_lists(msbfs_pkg, name):
    """The padded graphs of the prefix and LDS-hub cases: the planner sees more than 2^22
    vertices, the lists hold the uniform core only, and the first pull level's narrow list (what
    it leaves active, less the vertices of degree >= 32) is as long as the largest case needs."""
    m = msbfs_pkg
    assert set(_PADDED) == set(bl.PADDED)
    nd = _PADDED[name]
    core, padded = bl.padded_graph(m, name)
    assert padded.n == bl.PAD_N > 32768 * 32 * 4 and padded.n > 14336 * 32 * 4
    # the small-hub padding: the same core, between the two bounds of the planner
    small = bl.padded_graph(m, name, bl.PAD_HUB)[1]
    assert 14336 * 32 * 4 < small.n == bl.PAD_HUB <= 32768 * 32 * 4
    assert np.array_equal(small.rowptr[:core.n + 1], core.rowptr) and small.nnz == core.nnz
    assert np.array_equal(padded.rowptr[:core.n + 1], core.rowptr)
    assert (padded.rowptr[core.n:] == core.rowptr[-1]).all() and padded.col is not None
    assert np.array_equal(padded.col, core.col)
    deg = np.diff(core.rowptr)
    assert deg.min() > 0 and deg.max() < 1024
    qs = bl.queries(m, core.n, bl.GROUPS[1])
    lc = bl.level_counts(core, m.cpu_bfs(core, qs, distances=True).dist)
    narrow = lc[3][1] - int((deg >= bl.WIDE_DEFAULT).sum())
    print(name, "need", nd, "levels", lc, "narrow list left by level 2", narrow)
    assert narrow >= nd, (name, narrow, nd)
    assert lc[4][1] >= nd, (name, lc[4], nd)  # (hub_all_levels: level 3 leaves as many)
