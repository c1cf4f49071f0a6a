"""Locality key of the degree relabelling (device_graph_relabel_by_degree): on skewed graphs
vertices of equal degree are ordered by the rank of their highest-degree neighbour, then by id.
MSBFS_RELABEL_LOCALITY=0|1 forces the key off or on. Checked here: the map against a numpy
oracle, the regeneration path against the row gather, every solver's F and edge counts against
the CPU oracle with the key off and on, unchanged maps on graphs that are not skewed, and that
two relabels of one graph agree."""
import numpy as np
import pytest

from degree_graphs import _oracle_map

pytestmark = pytest.mark.gpu

VAR = "MSBFS_RELABEL_LOCALITY"


def _relabelled(make, monkeypatch, locality, regen=None):
    if locality is None:
        monkeypatch.delenv(VAR, raising=False)
    else:
        monkeypatch.setenv(VAR, str(locality))
    if regen is None:
        monkeypatch.delenv("MSBFS_RELABEL_REGEN", raising=False)
    else:
        monkeypatch.setenv("MSBFS_RELABEL_REGEN", str(regen))
    g = make()
    g.relabel_by_degree()
    return g


@pytest.mark.parametrize("scale", [14, 15])
def test_map_matches_numpy_oracle(msbfs_pkg, monkeypatch, scale):
    m = msbfs_pkg
    monkeypatch.setenv(VAR, "1")
    dg = m.DeviceGraph.rmat(scale, 16, 5, device=0)
    host = dg.download()
    want, deg = _oracle_map(host)
    dg.relabel_by_degree()
    o2n = dg.relabel_map()
    assert np.array_equal(o2n, want)
    r = dg.download()
    ndeg = np.diff(r.rowptr)
    assert np.all(np.diff(ndeg) <= 0)
    assert np.array_equal(deg, ndeg[o2n])
    for v in range(0, dg.n, 97):
        assert np.all(np.diff(r.col[r.rowptr[v]:r.rowptr[v + 1]]) >= 0)
    # the key changes the order at all (a map equal to the degree-only one would pass nothing)
    off = _relabelled(lambda: m.DeviceGraph.rmat(scale, 16, 5, device=0), monkeypatch, 0)
    assert not np.array_equal(off.relabel_map(), o2n)
    dg.close()
    off.close()


@pytest.mark.parametrize("kind", ["rmat", "uniform"])
def test_regeneration_matches_gather(msbfs_pkg, monkeypatch, kind):
    m = msbfs_pkg
    make = ((lambda: m.DeviceGraph.rmat(15, 16, 9, device=0)) if kind == "rmat"
            else (lambda: m.DeviceGraph.uniform(30000, 250000, 4, device=0)))
    a = _relabelled(make, monkeypatch, 1)
    b = _relabelled(make, monkeypatch, 1, regen=1)
    assert np.array_equal(a.relabel_map(), b.relabel_map())
    if kind == "uniform":  # forced on by the variable alone: the key is really in use
        host = make().download()
        assert np.array_equal(a.relabel_map(), _oracle_map(host)[0])
    ga, gb = a.download(), b.download()
    assert np.array_equal(ga.rowptr, gb.rowptr)
    assert np.array_equal(ga.col, gb.col)
    a.close()
    b.close()


@pytest.fixture(scope="module")
def answers(msbfs_pkg):
    """RMAT-14 in its original ids, the query sets and the CPU oracle's results, computed once."""
    m = msbfs_pkg
    dg = m.DeviceGraph.rmat(14, 16, 5, device=0)
    host = dg.download()
    dg.close()
    out = {}
    for K in (300, 520, 5):
        qs = m.QuerySet.random(host.n, K, 6, seed=2)
        out[K] = (qs, m.cpu_bfs(host, qs, count_edges=True))
    return out


@pytest.mark.parametrize("algo,K", [("bitpar", 300), ("bitpar", 520), ("dist", 5), ("sweep", 5)])
def test_same_answers_off_and_on(msbfs_pkg, monkeypatch, answers, algo, K):
    m = msbfs_pkg
    qs, ref = answers[K]
    got = []
    for locality in (0, 1):
        dg = _relabelled(lambda: m.DeviceGraph.rmat(14, 16, 5, device=0), monkeypatch, locality)
        with m.Solver(dg, algo, max_groups=qs.K) as s:
            r = s.run(qs, count_edges=True)
        assert np.array_equal(r.F, ref.F)
        assert np.array_equal(r.edges, ref.edges)
        got.append(r)
        dg.close()
    assert np.array_equal(got[0].F, got[1].F)
    assert np.array_equal(got[0].edges, got[1].edges)


@pytest.mark.parametrize("kind", ["uniform", "grid"])
def test_non_skewed_graphs_keep_their_order(msbfs_pkg, monkeypatch, kind):
    m = msbfs_pkg
    make = ((lambda: m.DeviceGraph.uniform(30000, 250000, 4, device=0)) if kind == "uniform"
            else (lambda: m.Graph.grid(60, 60, 0.9, 0, 2).to_device(0)))
    default = _relabelled(make, monkeypatch, None)
    off = _relabelled(make, monkeypatch, 0)
    assert np.array_equal(default.relabel_map(), off.relabel_map())
    default.close()
    off.close()


def test_deterministic_and_on_by_default_for_rmat(msbfs_pkg, monkeypatch):
    m = msbfs_pkg
    make = lambda: m.DeviceGraph.rmat(15, 16, 9, device=0)  # noqa: E731
    a = _relabelled(make, monkeypatch, None)
    b = _relabelled(make, monkeypatch, None)
    on = _relabelled(make, monkeypatch, 1)
    assert np.array_equal(a.relabel_map(), b.relabel_map())
    assert np.array_equal(a.relabel_map(), on.relabel_map())
    for g in (a, b, on):
        g.close()
