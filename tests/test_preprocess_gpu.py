"""Graph preprocessing on the device (csrc/src/kernels/gen.hip), whole arrays against numpy: the CSR
build by every way onto the device, the row sort, the degree relabelling, the streamed file
upload in pieces, and the range checks of the two edge-list builds. Then every solver on the same
graph. The graph (tests/degree_graphs.py) has one vertex at each degree the kernels branch on,
one below and one above; its oracles are checked against the host code in
tests/test_degree_graphs_cpu.py. All comparisons are integer equality."""
import struct
import types

import numpy as np
import pytest

from degree_graphs import (DEFAULT_DEGREES, boundary_graph, relabel_oracle, rows_ascending,
                           sorted_csr)

pytestmark = pytest.mark.gpu

WAYS = ("to_device", "from_file", "from_device_edges", "wrap")
LOCALITY = "MSBFS_RELABEL_LOCALITY"
PIECE, RESIDENT = "MSBFS_EDGE_PIECE", "MSBFS_EDGE_RESIDENT"


def _case(m, n, u, v, path, hubs=None):
    """a graph, its file and its oracles (read-only, shared by the tests of this module)"""
    u, v = np.asarray(u, np.int32), np.asarray(v, np.int32)
    host = m.Graph.from_edges(n, u, v)
    host.write(str(path))
    rowptr, col = sorted_csr(n, u, v)
    c = types.SimpleNamespace(n=n, u=u, v=v, hubs=hubs, host=host, path=str(path), rowptr=rowptr,
                              col=col, deg=np.diff(rowptr), _rel={})
    for a in (u, v, rowptr, col, host.rowptr, host.col):
        a.setflags(write=False)
    c.max_degree = int(c.deg.max()) if n else 0
    c.isolated = int((c.deg == 0).sum())

    def relabelled(locality):
        if locality not in c._rel:
            c._rel[locality] = relabel_oracle(host, locality)
        return c._rel[locality]
    c.relabelled = relabelled
    return c


def _boundary_case(m, path, seed):
    """the boundary graph, with the parent search's bound at -1, 0, +1 too. A vertex that is alone
    in its degree class keeps its rank whatever its locality key is, so the two sides of the
    short / long key kernels (256, 257) get four more hubs each: their order is the key's doing."""
    w = int(m.native.lib().msbfs_parents_wide_degree())
    degrees = list(DEFAULT_DEGREES)
    degrees += [d for d in (w - 1, w, w + 1) if d not in degrees]
    degrees += [256, 257] * 4
    n, u, v, hubs = boundary_graph(degrees, seed=seed)
    c = _case(m, n, u, v, path, hubs)
    c.degrees = degrees
    assert np.array_equal(c.deg[hubs], degrees) and n % 64 != 0
    o2n = c.relabelled(True)[0]
    for d in (256, 257):   # (equal keys would leave them in id order)
        same = np.sort(hubs[np.array(degrees) == d])
        assert len(same) == 5 and not (np.diff(o2n[same]) > 0).all(), d
    return c


@pytest.fixture(scope="module")
def B(msbfs_pkg, tmp_path_factory):
    return _boundary_case(msbfs_pkg, tmp_path_factory.mktemp("boundary") / "g.bin", 1)


@pytest.fixture(scope="module")
def B2(msbfs_pkg, tmp_path_factory):
    """the same degrees under another scramble of the ids"""
    return _boundary_case(msbfs_pkg, tmp_path_factory.mktemp("boundary2") / "g.bin", 2)


def _build(m, c, way):
    import torch
    dev = torch.device("cuda:0")
    if way == "to_device":
        return c.host.to_device(0)
    if way == "from_file":
        return m.DeviceGraph.from_file(c.path, device=0)
    if way == "from_device_edges":
        return m.DeviceGraph.from_device_edges(c.n, torch.from_numpy(c.u.copy()).to(dev),
                                               torch.from_numpy(c.v.copy()).to(dev), device=0)
    return m.DeviceGraph.wrap(c.n, torch.from_numpy(c.host.rowptr.copy()).to(dev),
                              torch.from_numpy(c.host.col.copy()).to(dev), device=0)


def _first_diff(a, b):
    i = int(np.flatnonzero(a != b)[0])
    return f"first difference at {i}: {a[i]} != {b[i]} ({int((a != b).sum())} differ)"


def _same_arrays(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b), f"{what}: {_first_diff(a, b)}"


def _check_build(c, dg, what):
    assert (dg.n, dg.nnz, dg.m) == (c.n, len(c.col), len(c.u)), what
    assert (dg.max_degree, dg.isolated) == (c.max_degree, c.isolated), what
    d = dg.download()
    _same_arrays(d.rowptr, c.rowptr, what + " rowptr")
    _same_arrays(rows_ascending(d.rowptr, d.col), c.col, what + " rows as multisets")


def _check_sort(c, dg, what):
    dg.sort_rows()
    d = dg.download()
    _same_arrays(d.rowptr, c.rowptr, what + " rowptr after sort_rows")
    _same_arrays(d.col, c.col, what + " col after sort_rows")
    dg.sort_rows()
    d = dg.download()
    _same_arrays(d.rowptr, c.rowptr, what + " rowptr after the second sort_rows")
    _same_arrays(d.col, c.col, what + " col after the second sort_rows")


def _check_relabel(c, dg, locality, what):
    o2n, rowptr, col = c.relabelled(locality)
    assert not dg.relabelled
    dg.relabel_by_degree()
    assert dg.relabelled
    _same_arrays(dg.relabel_map(), o2n, what + " old2new")
    d = dg.download()
    _same_arrays(d.rowptr, rowptr, what + " relabelled rowptr")
    _same_arrays(d.col, col, what + " relabelled col")
    assert (dg.n, dg.nnz, dg.m) == (c.n, len(c.col), len(c.u)), what
    assert (dg.max_degree, dg.isolated) == (c.max_degree, c.isolated), what
    assert dg.hybrid_extent() == c.n - c.isolated, what


# ---- the boundary graph: build, sort, relabel ---------------------------------------------------
@pytest.mark.parametrize("way", WAYS)
def test_build_and_sort_rows(msbfs_pkg, monkeypatch, B, way):
    monkeypatch.delenv(PIECE, raising=False)
    monkeypatch.delenv(RESIDENT, raising=False)
    dg = _build(msbfs_pkg, B, way)
    _check_build(B, dg, way)
    _check_sort(B, dg, way)
    dg.close()


@pytest.mark.parametrize("locality", [0, 1, None])
@pytest.mark.parametrize("way", WAYS)
def test_relabel_by_degree(msbfs_pkg, monkeypatch, B, way, locality):
    """unset: the graph is skewed (max degree 20001, mean 2), so the key is on"""
    if locality is None:
        monkeypatch.delenv(LOCALITY, raising=False)
    else:
        monkeypatch.setenv(LOCALITY, str(locality))
    dg = _build(msbfs_pkg, B, way)
    _check_relabel(B, dg, locality != 0, f"{way} locality={locality}")
    dg.close()
    a, b = B.relabelled(False)[0], B.relabelled(True)[0]
    assert not np.array_equal(a, b)   # (the key decides something on this graph)


def test_relabel_keys_are_computed_not_inherited(msbfs_pkg, monkeypatch, B, B2):
    """A locality key that no kernel wrote is read from whatever its buffer held, and after a
    relabelling of the same graph that is the right value. Two scrambles of one degree list
    alternate here, so that a key left over from the graph before is a wrong one."""
    monkeypatch.setenv(LOCALITY, "1")
    assert B.n == B2.n and not np.array_equal(B.relabelled(True)[0], B2.relabelled(True)[0])
    for i, c in enumerate((B, B2, B, B2)):
        dg = _build(msbfs_pkg, c, "to_device")
        _check_relabel(c, dg, True, f"graph {i}")
        dg.close()


# ---- edge cases, as graphs of their own ----------------------------------------------------------
def _edge_graphs():
    star = 37   # n = 65: one hub of degree 64 (the last row of the one-lane-per-row sort)
    leaves = np.array([x for x in range(65) if x != star])
    pairs = np.random.default_rng(4).permutation(131)[:120].reshape(2, 60)
    return {
        "one_vertex": (1, [], []),
        "one_self_loop": (1, [0], [0]),
        "hub_of_64": (65, np.full(64, star), leaves[::-1]),
        "degrees_up_to_1": (131, pairs[0], pairs[1]),   # 60 two-vertex components, 11 isolated
    }


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("name", list(_edge_graphs()))
def test_edge_case_graphs(msbfs_pkg, monkeypatch, tmp_path, name, way):
    m = msbfs_pkg
    n, u, v = _edge_graphs()[name]
    c = _case(m, n, u, v, tmp_path / "g.bin")
    expect = {"one_vertex": (0, 1), "one_self_loop": (2, 0), "hub_of_64": (64, 0),
              "degrees_up_to_1": (1, 11)}[name]
    assert (c.max_degree, c.isolated) == expect
    dg = _build(m, c, way)
    _check_build(c, dg, f"{name} {way}")
    _check_sort(c, dg, f"{name} {way}")
    dg.close()
    for locality in (0, 1):
        monkeypatch.setenv(LOCALITY, str(locality))
        dg = _build(m, c, way)
        _check_relabel(c, dg, locality != 0, f"{name} {way} locality={locality}")
        dg.close()


# ---- the streamed upload of a graph file ---------------------------------------------------------
def _pieces(mm):
    # one piece; two with a one-edge tail; two even ones; many, the last one partial (both)
    return [mm, mm - 1, (mm + 1) // 2, 1000, 999]


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("piece", range(5))
def test_streamed_file_in_pieces(msbfs_pkg, monkeypatch, B, piece, resident):
    mm = len(B.u)
    p = _pieces(mm)[piece]
    assert mm % 1000 and mm % 999 and mm > 2000
    monkeypatch.setenv(PIECE, str(p))
    monkeypatch.setenv(RESIDENT, str(resident))
    dg = msbfs_pkg.DeviceGraph.from_file(B.path, device=0)
    _check_build(B, dg, f"piece={p} resident={resident}")
    dg.close()


def _write_raw_graph(path, n, u, v):
    with open(path, "wb") as f:
        f.write(struct.pack("<iq", n, len(u)))
        f.write(np.stack([u, v], axis=1).astype("<i4").tobytes())


@pytest.fixture(scope="module")
def small_edges():
    rng = np.random.default_rng(8)
    n = 300
    return n, rng.integers(0, n, 2500).astype(np.int32), rng.integers(0, n, 2500).astype(np.int32)


@pytest.mark.parametrize("resident", [0, 1])
def test_streamed_file_errors_name_the_global_edge(msbfs_pkg, monkeypatch, tmp_path, small_edges,
                                                    resident):
    m = msbfs_pkg
    n, u, v = small_edges
    monkeypatch.setenv(PIECE, "1000")
    monkeypatch.setenv(RESIDENT, str(resident))
    p = str(tmp_path / "g.bin")
    _write_raw_graph(p, n, u, v)
    dg = m.DeviceGraph.from_file(p)   # the file itself is fine
    rowptr, col = sorted_csr(n, u, v)
    d = dg.download()
    _same_arrays(d.rowptr, rowptr, "rowptr")
    _same_arrays(rows_ascending(d.rowptr, d.col), col, "rows")
    dg.close()
    # one bad id in the third piece
    for bad_u, bad_v in ((n, 0), (0, -1), (2 ** 31 - 1, 5)):
        u1, v1 = u.copy(), v.copy()
        u1[2100], v1[2100] = bad_u, bad_v
        _write_raw_graph(p, n, u1, v1)
        with pytest.raises(m.native.MsbfsError,
                           match=r"edge 2100 has a vertex id outside \[0, n\)"):
            m.DeviceGraph.from_file(p)
    # bad ids in the first and the third piece: the lowest edge is named
    u1, v1 = u.copy(), v.copy()
    v1[2400] = n
    u1[500] = -7
    v1[7] = n + 1
    _write_raw_graph(p, n, u1, v1)
    with pytest.raises(m.native.MsbfsError, match=r"edge 7 has a vertex id outside \[0, n\)"):
        m.DeviceGraph.from_file(p)
    # and the next build is untouched by the failed ones
    _write_raw_graph(p, n, u, v)
    dg = m.DeviceGraph.from_file(p)
    d = dg.download()
    _same_arrays(rows_ascending(d.rowptr, d.col), col, "rows after the errors")
    dg.close()


@pytest.mark.parametrize("piece", ["0", "-5", "1", "99999999999", ""])
def test_piece_size_is_clamped(msbfs_pkg, monkeypatch, tmp_path, small_edges, piece):
    """below 1 means 1 (every edge its own piece), above 2^25 and empty mean the default"""
    n, u, v = small_edges
    u, v = u[:150], v[:150]
    p = str(tmp_path / "g.bin")
    _write_raw_graph(p, n, u, v)
    rowptr, col = sorted_csr(n, u, v)
    for resident in (0, 1):
        monkeypatch.setenv(PIECE, piece)
        monkeypatch.setenv(RESIDENT, str(resident))
        dg = msbfs_pkg.DeviceGraph.from_file(p)
        d = dg.download()
        _same_arrays(d.rowptr, rowptr, "rowptr")
        _same_arrays(rows_ascending(d.rowptr, d.col), col, "rows")
        dg.close()


# ---- edge arrays in device memory ----------------------------------------------------------------
def test_from_device_edges_checks_its_arguments(msbfs_pkg, small_edges):
    import torch
    m = msbfs_pkg
    n, u, v = small_edges
    du, dv = torch.from_numpy(u).to("cuda:0"), torch.from_numpy(v).to("cuda:0")
    with pytest.raises(TypeError):
        m.DeviceGraph.from_device_edges(n, du.to(torch.int64), dv.to(torch.int64))
    with pytest.raises(TypeError):
        m.DeviceGraph.from_device_edges(n, u, v)
    with pytest.raises(ValueError):
        m.DeviceGraph.from_device_edges(n, du.cpu(), dv.cpu())
    with pytest.raises(ValueError):
        m.DeviceGraph.from_device_edges(n, du, dv[:-1])
    with pytest.raises(ValueError):
        m.DeviceGraph.from_device_edges(n, du.reshape(50, 50), dv.reshape(50, 50))
    e = torch.empty(0, dtype=torch.int32, device="cuda:0")
    dg = m.DeviceGraph.from_device_edges(5, e, e)
    assert (dg.n, dg.nnz, dg.m, dg.max_degree, dg.isolated) == (5, 0, 0, 0, 5)
    d = dg.download()
    assert np.array_equal(d.rowptr, np.zeros(6, np.int64)) and len(d.col) == 0
    dg.close()
    # strided views are gathered first; relabel=True relabels
    rowptr, col = sorted_csr(n, u[::2], v[::2])
    dg = m.DeviceGraph.from_device_edges(n, du[::2], dv[::2], relabel=True)
    assert dg.relabelled and dg.m == 1250
    o2n = dg.relabel_map()
    r2, c2 = sorted_csr(n, o2n[u[::2]], o2n[v[::2]])
    d = dg.download()
    _same_arrays(d.rowptr, r2, "rowptr")
    _same_arrays(d.col, c2, "col")
    dg.close()


def test_from_device_edges_refuses_ids_out_of_range(msbfs_pkg, small_edges):
    """the kernel skips such an edge (nothing is written out of range) and the build fails after
    the count pass with the lowest offending edge index"""
    import torch
    m = msbfs_pkg
    n, u, v = small_edges

    def build(changes):
        u1, v1 = u.copy(), v.copy()
        for i, (a, b) in changes.items():
            u1[i], v1[i] = a, b
        return m.DeviceGraph.from_device_edges(n, torch.from_numpy(u1).to("cuda:0"),
                                               torch.from_numpy(v1).to("cuda:0"))

    for changes, first in (({5: (-1, 3)}, 5), ({9: (3, n)}, 9), ({2499: (n, n)}, 2499),
                           ({0: (2 ** 31 - 1, 0)}, 0), ({1800: (0, -1), 700: (n + 9, 1)}, 700)):
        with pytest.raises(m.native.MsbfsError,
                           match=rf"edge {first} has a vertex id outside \[0, n\)"):
            build(changes)
    dg = build({})
    rowptr, col = sorted_csr(n, u, v)
    d = dg.download()
    _same_arrays(d.rowptr, rowptr, "rowptr")
    _same_arrays(rows_ascending(d.rowptr, d.col), col, "rows")
    dg.close()


# ---- the solvers on the boundary graph -----------------------------------------------------------
DIRS = ("", "TBBBBBBBBBBBBBBBBBBBBBBBBBBBBB", "TBTBTBTBTBTBTBTBTBTBTBTBTBTBTB")
_REF = {}


def _queries(m, B, K):
    """hubs (every one of them alone in the first groups), leaves, both ends of two-vertex
    components, isolated vertices, ids outside [0, n), an empty group; then random mixtures"""
    n, g = B.n, B.host
    leaves = np.flatnonzero(B.deg == 1)
    k2 = leaves[B.deg[g.col[g.rowptr[leaves]]] == 1]
    iso = np.flatnonzero(B.deg == 0)
    two = np.flatnonzero(B.deg == 2)
    groups = [[int(h)] for h in B.hubs]
    groups += [[int(leaves[0])], [int(k2[0])], [int(k2[1]), int(g.col[g.rowptr[k2[1]]])],
               [int(iso[0])], [-1, n, n + 70, 2 ** 31 - 1], [], [int(two[0])],
               [int(B.hubs[0]), int(B.hubs[-1]), n], [int(iso[1]), int(leaves[5]), -3],
               [int(k2[2]), int(B.hubs[15])], [int(leaves[9]), int(leaves[9])]]
    rng = np.random.default_rng(K)
    pools = [B.hubs, leaves, two, k2, iso, np.array([-1, n, n + 1])]
    while len(groups) < K:
        groups.append([int(rng.choice(pools[int(rng.integers(len(pools)))]))
                       for _ in range(int(rng.integers(1, 4)))])
    return m.QuerySet.from_groups(groups[:K])


def _five(B):
    """of _queries: a hub; a leaf; both ends of a two-vertex component; an isolated vertex, a
    leaf and an invalid id; the two end hubs and an invalid id"""
    H = len(B.hubs)
    return np.array([16, H, H + 2, H + 8, H + 7])


def _ref(m, B, K):
    if K not in _REF:
        qs = _queries(m, B, K)
        _REF[K] = (qs, m.cpu_bfs(B.host, qs, count_edges=True))
    return _REF[K]


@pytest.fixture(scope="module")
def devs(msbfs_pkg, B):
    """the boundary graph on the device, as built and relabelled (the default: key on)"""
    plain = B.host.to_device(0)
    rel = B.host.to_device(0).relabel_by_degree()
    yield {False: plain, True: rel}
    plain.close()
    rel.close()


def _assert_F(r, ref, what, edges=True):
    assert np.array_equal(r.F, ref.F), (what, np.flatnonzero(r.F != ref.F)[:8],
                                        r.F[r.F != ref.F][:8], ref.F[r.F != ref.F][:8])
    if edges:
        assert np.array_equal(r.edges, ref.edges), (what, np.flatnonzero(r.edges != ref.edges)[:8])


@pytest.mark.parametrize("dirs", DIRS)
@pytest.mark.parametrize("K", [64, 1024])
@pytest.mark.parametrize("relabel", [False, True])
def test_bitpar_on_the_boundary_graph(msbfs_pkg, B, devs, relabel, K, dirs):
    m = msbfs_pkg
    qs, ref = _ref(m, B, K)
    assert ref.F[0] > 0 and ref.F.max() > 10 * B.n   # (a path of hubs: deep and wide)
    with m.Solver(devs[relabel], "bitpar", max_groups=K,
                  tuning=("leaf=0" + (",dirs=" + dirs if dirs else ""))) as s:
        r = s.run(qs, count_edges=True)
        _assert_F(r, ref, f"relabel={relabel} K={K} dirs={dirs}")
        tr = [t for t in s.level_trace() if t["batch"] == 0]
    if dirs:   # the hubs were pulled, not only pushed (level L follows dirs[L - 1])
        forced = [t for t in tr if t["level"] <= len(dirs)]
        assert len(forced) > 20, tr
        assert all(t["dir"] == dirs[t["level"] - 1] for t in forced), tr


@pytest.mark.parametrize("dirs", DIRS)
@pytest.mark.parametrize("K", [64, 1024])
@pytest.mark.parametrize("leaf", [0, 1])
def test_bitpar_leaf_fold_on_the_boundary_graph(msbfs_pkg, B, devs, leaf, K, dirs):
    m = msbfs_pkg
    qs, ref = _ref(m, B, K)
    with m.Solver(devs[True], "bitpar", max_groups=K,
                  tuning=(f"leaf={leaf}" + (",dirs=" + dirs if dirs else ""))) as s:
        r = s.run(qs)
    _assert_F(r, ref, f"leaf={leaf} K={K} dirs={dirs}", edges=False)
    assert r.stats["leaf_folded"] == (int((B.deg == 1).sum()) if leaf else 0)


def test_bitpar_folds_leaves_by_itself_here(msbfs_pkg, B, devs):
    """three quarters of the vertices are leaves: above the share at which folding turns on"""
    m = msbfs_pkg
    qs, ref = _ref(m, B, 64)
    with m.Solver(devs[True], "bitpar", max_groups=64) as s:
        r = s.run(qs)
    _assert_F(r, ref, "default tuning", edges=False)
    assert r.stats["leaf_folded"] == int((B.deg == 1).sum())


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("algo", ["dist", "topdown", "sweep"])
def test_per_group_solvers_on_the_boundary_graph(msbfs_pkg, B, devs, algo, relabel):
    m = msbfs_pkg
    qs, ref = _ref(m, B, 64)
    pick = _five(B)
    sub = qs.subset(pick)
    with m.Solver(devs[relabel], algo, max_groups=sub.K) as s:
        r = s.run(sub, count_edges=True)
    assert np.array_equal(r.F, ref.F[pick]) and np.array_equal(r.edges, ref.edges[pick]), \
        (algo, relabel, r.F, ref.F[pick], r.edges, ref.edges[pick])


@pytest.fixture(scope="module")
def matrices(msbfs_pkg, B):
    """cpu_bfs distances of the 64 groups on the host graph"""
    qs, ref = _ref(msbfs_pkg, B, 64)
    r = msbfs_pkg.cpu_bfs(B.host, qs, distances=True)
    assert np.array_equal(r.F, ref.F)
    r.dist.setflags(write=False)
    return qs, r.dist


@pytest.mark.parametrize("relabel", [False, True])
def test_distances_on_the_boundary_graph(msbfs_pkg, B, devs, matrices, relabel):
    m = msbfs_pkg
    qs, D = matrices
    with m.Solver(devs[relabel], "bitpar", max_groups=qs.K) as s:
        r = s.distances(qs)
    _same_arrays(r.dist, D, f"dist relabel={relabel}")
    assert np.array_equal(r.F, np.where(D >= 0, D, 0).sum(axis=1, dtype=np.int64))


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("algo,K", [("bitpar", 64), ("dist", 5), ("topdown", 5), ("sweep", 5)])
def test_parents_on_the_boundary_graph(msbfs_pkg, B, devs, matrices, algo, K, relabel):
    """the README's rule: the first neighbour one level nearer, in the device row order"""
    from test_parents_gpu import _same
    m = msbfs_pkg
    qs, D = matrices
    pick = np.arange(64) if K == 64 else _five(B)
    sub = qs.subset(pick)
    dg = devs[relabel]
    with m.Solver(dg, algo, max_groups=sub.K) as s:
        r = s.parents(sub)
    _same(r, B.host, dg, D[pick], f"{algo} relabel={relabel}")
    if not relabel:   # the device rows in the original ids: cpu_bfs on them gives the same matrix
        ref = m.cpu_bfs(dg.download(), sub, parents=True)
        _same_arrays(ref.dist, D[pick], "cpu dist")
        _same_arrays(r.parent, ref.parent, f"{algo} parent against cpu_bfs")
