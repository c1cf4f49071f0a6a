"""The inputs of test_prefix_level_gpu.py meet every boundary of the first pull level, shown on the
inputs alone (prefix_graphs.census: levels 1 and 2 of every group from sparse products; the
internal ids from the numpy oracle of the degree relabelling, locality key on). These are
conditions on the committed inputs, not measurements. No GPU."""
import numpy as np
import pytest

import block_loops as bl
import prefix_graphs as pg
from degree_graphs import relabel_oracle

KS = (64, 128, 256, 512, 1024)


@pytest.fixture(scope="module")
def design(msbfs_pkg):
    m = msbfs_pkg
    g = pg.boundary_graph(1)
    core, padded = pg.host_graphs(m, g)
    o2n = relabel_oracle(padded, locality=True)[0]
    qs = pg.boundary_queries(m, g, o2n, 1024)
    return m, g, core, padded, o2n, qs


def test_shape(design):
    m, g, core, padded, o2n, qs = design
    deg = np.diff(padded.rowptr)
    assert padded.n == pg.PAD_N == bl.PAD_N and g.n_core == core.n
    assert int((deg >= 3).sum()) == pg.H            # the body: internal ids [0, H)
    assert int((deg == 2).sum()) >= 2048            # the tail: ids from H on
    assert int((deg == 1).sum()) >= 1024
    assert int((deg > 0).sum()) == g.n_core and g.n_core % 32 != 0
    assert not (deg[g.n_core:] > 0).any()
    # leaves hang on body and on tail vertices
    leaves = np.flatnonzero(deg == 1)
    par = deg[padded.col[padded.rowptr[leaves]]]
    assert (par >= 3).any() and (par == 2).any()
    # one self-loop, one duplicate edge
    u, v = g.u.astype(np.int64), g.v.astype(np.int64)
    assert int((u == v).sum()) == 1
    key = np.minimum(u, v) * g.n + np.maximum(u, v)
    assert len(key) - len(np.unique(key)) == 1
    # the relabelling keeps the classes in id ranges whatever its tie-break
    d2 = np.empty(padded.n, np.int64)
    d2[o2n] = deg
    assert d2[:pg.H].min() >= 3 and (d2[pg.H:pg.H + int((deg == 2).sum())] == 2).all()


def test_groups_are_prefixes(design):
    m, g, core, padded, o2n, qs = design
    assert qs.K == 1024 and (np.diff(qs.off) > 0).all()
    for K in KS:
        assert pg.boundary_queries(m, g, o2n, K) == qs.subset(range(K))


@pytest.mark.parametrize("K", KS)
def test_census(design, K):
    """Every condition for the 1024 groups; for the first K of them every one that names no group
    above K - 1 (a row of 65 groups needs 128)."""
    m, g, core, padded, o2n, qs = design
    c = pg.census(g, o2n, qs.subset(range(K)))
    print(K, {k: v for k, v in c.items() if not k.startswith("rows_")})
    # ---- shape
    assert c["classes_are_ranges"] and c["body"] == pg.H and c["tail"] >= 2048
    assert c["leaves"] >= 1024 and c["n_core"] % 32 != 0
    for L in pg.PREFIX_LENGTHS:
        assert c["level2_by_plen"][L] >= 2, (L, c["level2_by_plen"])
    assert c["zero_run"] >= 96
    # ---- rows at the start of level 2, among body carriers and among tail pushers
    sizes = {1, 2, 3, 4} | ({65} if K >= 128 else set())
    for part in ("body", "tail"):
        assert sizes <= c["row_sizes_" + part], (part, c["row_sizes_" + part])
        missing = [sorted(s) for s in pg.required_row_sets(K) if s not in c["rows_" + part]]
        assert not missing, (part, missing)
        words = lambda s: len({k // 64 for k in s})
        if K >= 256:  # a 3-set in three 64-bit words
            assert any(len(s) == 3 and words(s) == 3 for s in c["rows_" + part]), part
        if K >= 128:  # a 4-set that spans words
            assert any(len(s) == 4 and words(s) > 1 for s in c["rows_" + part]), part
    if K == 1024:
        want = [{0}, {63}, {64}, {1023}, {63, 64}, {0, 1023}, {1021, 1022, 1023}]
        assert all(frozenset(s) in pg.required_row_sets(K) for s in want)
    # ---- positions: a carrier alone at entry 0, and alone at entry L - 1
    for L in pg.POSITIONAL:
        assert L in c["alone_first"] and L in c["alone_last"], (L, c["alone_first"], c["alone_last"])
        assert c["alone_first"][L] != c["alone_last"][L]
    assert pg.POSITIONAL == (pg.ROUND + 1, pg.BIG + 1, 2 * pg.BIG + 1)
    # ---- the bound
    assert c["at_H-1"] is not None and c["at_H"] is not None
    # ---- pushed only (prefix length 0, and a big vertex), pulled and pushed, other groups
    assert {0, pg.BIG + 1} <= c["push_only_plen"], c["push_only_plen"]
    assert c["same_group_both"] > 0 and c["other_groups"] > 0
    # ---- leaves
    assert c["pusher_with_leaf"] > 0 and c["level2_body_with_leaf"] > 0 and c["leaf_sources"] > 0


def test_sun(msbfs_pkg):
    m = msbfs_pkg
    s = pg.sun_graph()
    for g_ in bl.MAX_GRIDS:
        assert s.nbody >= pg.sun_need(g_) == bl.TILES_MIN * pg.TILE_WAVES * g_ * pg.VT
        assert s.nbody // pg.VT // (pg.TILE_WAVES * g_) >= bl.TILES_MIN
    core, padded = pg.host_graphs(m, s)
    deg = np.diff(padded.rowptr)
    assert padded.n == pg.PAD_N and int((deg >= 3).sum()) == s.nbody + 1 < pg.H
    assert deg[0] == s.nbody + pg.SUN_HANDLES > pg.BIG and (deg[1:s.nbody + 1] == 3).all()
    assert (deg[s.handles] == 2).all()
    # every body vertex (and every other handle) is at level 2 for every group: the level's
    # histogram entry is their count, for all 1024 groups
    qs = pg.sun_queries(m, s, 1024)
    assert qs.K == 1024 and pg.sun_queries(m, s, 256) == qs.subset(range(256))
    r = m.cpu_bfs(core, qs, profile=True, bins="all")
    assert (r.hist[:, 1] == 2).all()  # the hub and the handle's leaf
    assert (r.hist[:, 2] == s.nbody + pg.SUN_HANDLES - 1).all()
    # ... and exactly, for one group and for the last: the distances of the body
    D = m.cpu_bfs(core, qs.subset([0, 1023]), distances=True).dist
    assert (D[:, 1:s.nbody + 1] == 2).all() and (D[:, 0] == 1).all()
