"""The prescribed-degree generator and the preprocessing oracles of degree_graphs.py, held against
the host code (Graph.from_edges, cpu_bfs) and never against the kernels they are to judge."""
import numpy as np
import pytest

from degree_graphs import (DEFAULT_DEGREES, ISOLATED, K2_COMPONENTS, boundary_graph,
                           relabel_oracle, rows_ascending, sorted_csr)


def _degrees(n, u, v):
    return np.bincount(np.concatenate([u, v]), minlength=n)


@pytest.mark.parametrize("degrees", [
    DEFAULT_DEGREES,
    (1,), (2,), (3,), (700,),            # one hub: no path; the self-loop where it fits
    (1, 1), (2, 1), (3, 3), (1, 40),     # two hubs: the path edge uses a degree-1 hub up
    (1, 2, 1), (3, 4, 2), (2, 5, 3),     # three hubs: path + self-loop + duplicate use all up
    (5, 4, 4, 3, 2, 2, 2, 2, 2, 1),      # the 6th and 8th hubs have no room: others take the extras
    (64, 1024, 65, 1025, 17000),
])
def test_hubs_have_exactly_the_requested_degrees(degrees):
    n, u, v, hubs = boundary_graph(degrees, seed=3)
    assert u.dtype == np.int32 and v.dtype == np.int32 and len(u) == len(v)
    assert u.min() >= 0 and v.min() >= 0 and max(u.max(), v.max()) < n
    assert len(hubs) == len(degrees) == len(set(hubs.tolist()))
    deg = _degrees(n, u, v)
    assert np.array_equal(deg[hubs], np.asarray(degrees))
    assert n % 64 != 0
    assert int((deg == 0).sum()) in (ISOLATED, ISOLATED + 1)
    # the hubs are joined in the order given
    pairs = set(zip(u.tolist(), v.tolist())) | set(zip(v.tolist(), u.tolist()))
    assert all((int(a), int(b)) in pairs for a, b in zip(hubs[:-1], hubs[1:]))
    # components of two leaves
    rowptr, col = sorted_csr(n, u, v)
    leaf = np.flatnonzero(deg == 1)
    assert int((deg[col[rowptr[leaf]]] == 1).sum()) >= 2 * K2_COMPONENTS


def test_degree_below_the_path_edges_is_refused():
    with pytest.raises(ValueError):
        boundary_graph((5, 1, 5))
    with pytest.raises(ValueError):
        boundary_graph(())


def test_default_graph_shape():
    n, u, v, hubs = boundary_graph()
    deg = _degrees(n, u, v)
    assert (n, len(u)) == (110498, 110487)
    assert int((deg == 1).sum()) == 82845 and int((deg == 0).sum()) == ISOLATED
    assert 8 * int((deg == 1).sum()) > n          # the leaf fold's own threshold
    loops = np.flatnonzero(u == v)
    assert len(loops) == 1 and u[loops[0]] in hubs
    code = np.minimum(u, v).astype(np.int64) * n + np.maximum(u, v)
    dup = np.flatnonzero(np.bincount(np.unique(code, return_inverse=True)[1]) == 2)
    assert len(dup) == 1


def test_deterministic_per_seed():
    a, b, c = boundary_graph(seed=5), boundary_graph(seed=5), boundary_graph(seed=6)
    assert a[0] == b[0] == c[0]
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert not np.array_equal(a[1], c[1]) and not np.array_equal(a[3], c[3])


@pytest.fixture(scope="module")
def host(msbfs_pkg):
    n, u, v, hubs = boundary_graph()
    return msbfs_pkg.Graph.from_edges(n, u, v), u, v, hubs


def test_sorted_csr_matches_host_build(msbfs_pkg, host):
    g, u, v, _ = host
    rowptr, col = sorted_csr(g.n, u, v)
    assert rowptr.dtype == np.int64 and col.dtype == np.int32
    assert np.array_equal(rowptr, g.rowptr)
    assert np.array_equal(col, rows_ascending(g.rowptr, g.col))
    py = msbfs_pkg.Graph.from_edges(g.n, u, v, use_native=False)
    assert np.array_equal(rowptr, py.rowptr)
    assert np.array_equal(col, rows_ascending(py.rowptr, py.col))
    # every row really ascending (no entry crosses a row end)
    inner = np.ones(len(col), bool)
    inner[rowptr[1:-1][rowptr[1:-1] < len(col)]] = False
    assert (np.diff(col)[inner[1:]] >= 0).all()


def _queries(m, n, g, hubs):
    deg = np.diff(g.rowptr)
    leaves = np.flatnonzero(deg == 1)
    k2 = leaves[deg[g.col[g.rowptr[leaves]]] == 1]
    iso = np.flatnonzero(deg == 0)
    groups = [[int(hubs[0])], [int(hubs[-1])], [int(hubs[3]), int(hubs[17])], [int(leaves[0])],
              [int(k2[0])], [int(k2[1]), int(hubs[9])], [int(iso[0])], [-1, n, n + 5], [],
              [int(iso[1]), int(leaves[7]), n]]
    return m.QuerySet.from_groups(groups)


@pytest.mark.parametrize("locality", [False, True])
def test_relabel_oracle_keeps_every_answer(msbfs_pkg, host, locality):
    m = msbfs_pkg
    g, u, v, hubs = host
    o2n, rowptr, col = relabel_oracle(g, locality)
    n = g.n
    assert o2n.dtype == np.int32 and np.array_equal(np.sort(o2n), np.arange(n))
    deg = np.diff(g.rowptr)
    ndeg = np.diff(rowptr)
    assert np.array_equal(ndeg[o2n], deg) and (np.diff(ndeg) <= 0).all()
    # the hubs' degrees are distinct and ascending (the first one's, 2, is shared with spokes)
    assert np.array_equal(o2n[hubs[:0:-1]], np.arange(len(hubs) - 1))
    # the same graph: its edge list mapped through old2new has this sorted CSR
    r2, c2 = sorted_csr(n, o2n[u], o2n[v])
    assert np.array_equal(r2, rowptr) and np.array_equal(c2, col)
    rg = m.Graph(n, rowptr, col)
    qs = _queries(m, n, g, hubs)
    mapped = m.QuerySet.from_groups(
        [[int(o2n[x]) if 0 <= x < n else int(x) for x in qs.group(k)] for k in range(qs.K)])
    a = m.cpu_bfs(g, qs, count_edges=True)
    b = m.cpu_bfs(rg, mapped, count_edges=True)
    assert a.F[0] > 0 and a.F[6] == 0 and a.F[7] == 0
    assert np.array_equal(a.F, b.F) and np.array_equal(a.edges, b.edges)
    if locality:   # equal-degree vertices are grouped by their hub: not the degree-only order
        assert not np.array_equal(o2n, relabel_oracle(g, False)[0])
