"""BFS parents from every device solver, through Solver.parents / msbfs_solver_run_parents(_host).
Every result is held against (a) the exact expected matrix: D from the numpy distance oracle, the
device graph's download() and relabel_map() read after the run, and for every reached non-source
(k, v) the first entry of v's downloaded row whose user id lies at D[k, v] - 1; and (b) an
independent validity check on the original host graph (sources are self-parents, unreached
entries -1, (v, parent) an edge, the parent one level nearer). dist and F must equal the distance
oracle exactly.

The bit-parallel solver searches narrow vertices with one lane group and queues vertices from a
degree bound on for a block each (1024 row entries per step); the per-group solvers give such a
row to a whole wave. The bound is one constant of the build (kParentsWideDegree, 256), read here
through msbfs_parents_wide_degree(): the star below (centre degree 3000) lies on the wide side of
it, the grids (max degree <= 6) on the narrow side, the RMAT graphs on both."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 123456789


def _wide_bound(m):
    """the build's bound between the narrow and the wide parent search (see the module docstring)"""
    b = int(m.native.lib().msbfs_parents_wide_degree())
    assert b == 256
    return b


_ORACLE = {}
ALGOS = ("bitpar", "dist", "topdown", "sweep")


def _oracle(key, g, qs):
    """distance matrix of the numpy oracle, computed once per (graph, query set) key"""
    if key not in _ORACLE:
        from msbfs.ops.reference import bfs_dist_numpy
        D = np.full((qs.K, g.n), -1, dtype=np.int32)
        for k in range(qs.K):
            D[k] = bfs_dist_numpy(g.n, g.rowptr, g.col, qs.group(k))
        D.setflags(write=False)
        _ORACLE[key] = D
    return _ORACLE[key]


def _F_of(D):
    return np.where(D >= 0, D, 0).sum(axis=1, dtype=np.int64)


def _expected(dg, D):
    """(a), from the device graph as it is after the run"""
    h = dg.download()
    n = h.n
    o2n = dg.relabel_map() if dg.relabelled else np.arange(n, dtype=np.int32)
    n2o = np.empty(n, dtype=np.int64)
    n2o[o2n] = np.arange(n)
    deg = np.diff(h.rowptr)
    row_int = np.repeat(np.arange(n), deg)            # internal id of every entry's vertex
    pos = np.arange(len(h.col)) - h.rowptr[row_int]   # its position in the row
    row_usr, col_usr = n2o[row_int], n2o[h.col]
    K = D.shape[0]
    P = np.full((K, n), -1, dtype=np.int32)
    for k in range(K):
        d = D[k]
        ok = (d[row_usr] > 0) & (d[col_usr] == d[row_usr] - 1)
        first = np.full(n, np.iinfo(np.int64).max)     # by internal id
        np.minimum.at(first, row_int[ok], pos[ok])
        has = np.nonzero(d[n2o] > 0)[0]                # internal ids of reached non-sources
        assert (first[has] < deg[has]).all()
        P[k, n2o[has]] = col_usr[h.rowptr[:-1][has] + first[has]]
        src = np.nonzero(d == 0)[0]
        P[k, src] = src
    return P


_EDGESETS = {}


def _valid(g, D, P, what=""):
    """(b), on the original host graph"""
    n = g.n
    assert P is not None and P.dtype == np.int32 and P.shape == D.shape, what
    key = id(g)
    if key not in _EDGESETS:
        u = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.rowptr))
        _EDGESETS[key] = (g, np.unique(u * n + g.col))
    codes = _EDGESETS[key][1]
    cols = np.arange(n)[None, :]
    assert np.array_equal(P[D == 0], np.broadcast_to(cols, D.shape)[D == 0]), what
    assert (P[D < 0] == -1).all(), what
    rest = D > 0
    p = P[rest].astype(np.int64)
    assert ((p >= 0) & (p < n)).all(), what
    kk, vv = np.nonzero(rest)
    assert np.array_equal(D[kk, p], D[kk, vv] - 1), what
    assert np.isin(vv * n + p, codes).all(), what


def _same(r, g, dg, D, what=""):
    assert r.dist is not None and r.dist.dtype == np.int32 and r.dist.shape == D.shape, what
    if not np.array_equal(r.dist, D):
        k, v = np.argwhere(r.dist != D)[0]
        raise AssertionError(f"{what}: dist[{k}, {v}] = {r.dist[k, v]}, oracle {D[k, v]}")
    assert np.array_equal(r.F, _F_of(D)), what
    _valid(g, D, r.parent, what)
    E = _expected(dg, D)
    if not np.array_equal(r.parent, E):
        k, v = np.argwhere(r.parent != E)[0]
        raise AssertionError(f"{what}: parent[{k}, {v}] = {r.parent[k, v]}, expected {E[k, v]} "
                             f"({int((r.parent != E).sum())} entries differ)")
    return E


def _dev(g, relabel=False):
    dg = g.to_device(0)
    if relabel:  # degree-descending internal ids; queries and results keep the original ones
        dg.relabel_by_degree()
        assert dg.relabelled
    return dg


def _graphs(m):
    return [("rmat10", m.Graph.rmat(10, 16, 3)), ("rmat12", m.Graph.rmat(12, 8, 5)),
            ("uniform", m.Graph.uniform(3000, 9000, 11)), ("grid", m.Graph.grid(40, 60, 0.9, 5, 2))]


# ---- bit-parallel: word layouts, passes -----------------------------------------------------------
def _rmat11(m):
    g = m.Graph.rmat(11, 16, 9)
    qs = m.QuerySet.random(g.n, 1024, 2, seed=77)
    return g, qs, _oracle("rmat11", g, qs)


@pytest.mark.parametrize("K", [1, 64, 65, 300, 1024])
def test_bitpar_word_layouts(msbfs_pkg, K):
    """1 to 16 words; max degree 3225 (wide search) next to 336 isolated vertices"""
    m = msbfs_pkg
    g, qs, D = _rmat11(m)
    assert int(np.diff(g.rowptr).max()) >= _wide_bound(m)
    sub = qs.subset(np.arange(K))
    dg = g.to_device(0)
    with m.Solver(dg, "bitpar", max_groups=K) as s:
        _same(s.parents(sub), g, dg, D[:K], f"K={K}")


def test_bitpar_several_passes(msbfs_pkg):
    """K = 300 over passes of 128 groups: k0 > 0 and a partial last pass; host and device output,
    the padding of both matrices untouched"""
    import torch
    m = msbfs_pkg
    g, qs, D = _rmat11(m)
    n, ld = g.n, g.n + 7
    sub = qs.subset(np.arange(300))
    dg = g.to_device(0)
    with m.Solver(dg, "bitpar", max_groups=128) as s:
        r = s.parents(sub)
        assert r.stats["batches"] == 3
        E = _same(r, g, dg, D[:300], "host output")
        r1 = s.parents(sub, ld=ld)
        assert r1.dist.shape == (300, n) and r1.parent.shape == (300, n)
        assert np.array_equal(r1.dist, D[:300]) and np.array_equal(r1.parent, E)
        db = torch.full((300, ld), SENTINEL, dtype=torch.int32, device="cuda:0")
        pb = torch.full((300, ld), SENTINEL, dtype=torch.int32, device="cuda:0")
        r2 = s.parents(sub, dist_ptr=db.data_ptr(), parent_ptr=pb.data_ptr(), ld=ld)
        assert r2.dist is None and r2.parent is None and np.array_equal(r2.F, r.F)
        hd, hp = db.cpu().numpy(), pb.cpu().numpy()
        assert np.array_equal(hd[:, :n], D[:300]) and (hd[:, n:] == SENTINEL).all()
        assert np.array_equal(hp[:, :n], E) and (hp[:, n:] == SENTINEL).all()
        with pytest.raises(ValueError):
            s.parents(sub, dist_ptr=db.data_ptr())
        with pytest.raises(ValueError):
            s.parents(sub, parent_ptr=pb.data_ptr())
        with pytest.raises(ValueError):
            s.parents(sub, dist_ptr=db.data_ptr(), parent_ptr=pb.data_ptr(), ld=n - 1)


# ---- bit-parallel: the three recording sites ----------------------------------------------------
@pytest.mark.parametrize("force_dir,wide", [(1, 64), (2, 4), (0, 1)])
def test_bitpar_recording_sites(msbfs_pkg, force_dir, wide):
    """push only / pull with hub chunks / mixed"""
    m = msbfs_pkg
    for name, g in _graphs(m):
        qs = m.QuerySet.random(g.n, 200, 5, seed=3)
        D = _oracle(("sites", name), g, qs)
        dg = g.to_device(0)
        with m.Solver(dg, "bitpar", max_groups=qs.K, force_dir=force_dir, wide_degree=wide) as s:
            _same(s.parents(qs), g, dg, D, f"{name} force_dir={force_dir} wide={wide}")
            dirs = {t["dir"] for t in s.level_trace()}
        if force_dir == 1:
            assert dirs == {"T"}, name
        if force_dir == 2:
            assert "B" in dirs, name


def _push_batches(tr):
    """Lengths of the device-driven push batches in a level trace. A host-driven level has its
    own wall time; the levels of one batch share the batch's, split evenly: a run of push
    records with one ms value is a batch."""
    runs, i = [], 0
    while i < len(tr):
        j = i
        while j + 1 < len(tr) and tr[j + 1]["dir"] == "T" == tr[i]["dir"] \
                and tr[j + 1]["ms"] == tr[i]["ms"]:
            j += 1
        if j > i:
            runs.append(j - i + 1)
        i = j + 1
    return runs


@pytest.mark.parametrize("force_dir", [0, 1])
def test_bitpar_device_driven_push_batches(msbfs_pkg, force_dir):
    """A road-like grid: the push levels run in device-driven batches, whose closed levels must
    write nothing and commit nothing. Batches are enqueued with 4, 8, 16, 32, 64 levels; one that
    the trace shows shorter than it was enqueued ended in closed levels. With default options
    the first batch (4 enqueued) stops for a pull after fewer levels; push-only runs all 93
    levels in batches, and the last one (64 enqueued) holds the rest."""
    m = msbfs_pkg
    g = m.Graph.grid(40, 60, 0.9, 0, 2)
    assert int(np.diff(g.rowptr).max()) < _wide_bound(m)
    qs = m.QuerySet.random(g.n, 70, 2, seed=12)
    D = _oracle("gridbatch", g, qs)
    assert int(D.max()) > 64
    dg = g.to_device(0)
    with m.Solver(dg, "bitpar", max_groups=qs.K, force_dir=force_dir) as s:
        _same(s.parents(qs), g, dg, D, "grid")
        tr = s.level_trace()
    dirs = "".join(t["dir"] for t in tr)
    runs = _push_batches(tr)
    assert len(tr) >= int(D.max()) and dirs[0] == "T"
    assert runs and max(runs) <= 64, (dirs, runs)
    if force_dir == 1:
        assert set(dirs) == {"T"} and len(runs) >= 3 and sum(runs) >= 64, (dirs, runs)
        assert runs[-1] < 64, runs   # closed levels at the end of the last batch
    else:
        assert runs[0] < 4, runs     # the first batch stopped: its later levels were closed


# ---- narrow and wide search -------------------------------------------------------------------------
def _star(m):
    leaves = np.arange(1, 3001, dtype=np.int32)
    u = np.concatenate([np.zeros(3000, np.int32), np.array([3000], np.int32)])
    v = np.concatenate([leaves, np.array([3001], np.int32)])
    g = m.Graph.from_edges(3002, u, v, stable=True)  # (rows in edge order: 0's row is 1..3000)
    qs = m.QuerySet.from_groups([[3001], [2999, 5], [1]])
    return g, qs, _oracle("star", g, qs)


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
def test_star_wide_search(msbfs_pkg, algo, relabel):
    """centre 0 joined to leaves 1..3000, plus 3000-3001. From [3001] the centre's only parent,
    3000, is one entry of a 3000-entry row (the last one where the graph keeps its ids)."""
    m = msbfs_pkg
    g, qs, D = _star(m)
    assert int(np.diff(g.rowptr).max()) == 3000 >= _wide_bound(m)
    dg = _dev(g, relabel)
    with m.Solver(dg, algo, max_groups=qs.K) as s:
        r = s.parents(qs)
        _same(r, g, dg, D, f"star {algo} relabel={relabel}")
    assert r.parent[0, 0] == 3000 and r.parent[0, 3000] == 3001 and r.parent[0, 7] == 0
    assert r.parent[1, 0] in (5, 2999) and r.parent[2, 0] == 1
    if not relabel:
        h = dg.download()
        assert h.col[h.rowptr[1] - 1] == 3000 and h.rowptr[1] == 3000  # the row's last entry


# ---- relabelled graphs, all solvers on one graph ----------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_relabelled_graph_original_ids(msbfs_pkg, algo):
    m = msbfs_pkg
    for name, g in _graphs(m)[:3]:
        K = 130 if algo == "bitpar" else 9
        qs = m.QuerySet.random(g.n, K, 3, seed=21)
        D = _oracle(("relabel", name, K), g, qs)
        for relabel in (True, False):
            dg = _dev(g, relabel)
            with m.Solver(dg, algo, max_groups=K) as s:
                _same(s.parents(qs), g, dg, D, f"{name} {algo} relabel={relabel}")


@pytest.mark.parametrize("relabel", [False, True])
def test_all_solvers_agree_on_one_device_graph(msbfs_pkg, relabel):
    m = msbfs_pkg
    for name, g in _graphs(m):
        qs = m.QuerySet.random(g.n, 9, 3, seed=len(name))
        D = _oracle(("agree", name), g, qs)
        dg = _dev(g, relabel)
        got = []
        for algo in ALGOS:
            with m.Solver(dg, algo, max_groups=qs.K) as s:
                r = s.parents(qs)
                # a second call on the same solver: the lazy reset between groups and calls
                r2 = s.parents(qs.subset(np.arange(8, -1, -1)))
            assert np.array_equal(r2.parent, r.parent[::-1]) and np.array_equal(r2.dist, D[::-1])
            got.append(r.parent)
        _same(r, g, dg, D, f"{name} sweep")
        for algo, P in zip(ALGOS, got):
            assert np.array_equal(P, got[0]), (name, algo)


def test_multi_source_bfs_parents(msbfs_pkg):
    m = msbfs_pkg
    name, g = _graphs(m)[0]
    qs = m.QuerySet.random(g.n, 9, 3, seed=len(name))
    D = _oracle(("agree", name), g, qs)
    ref = m.cpu_bfs(g, qs, count_edges=True)
    for algo in ("auto", "bitpar", "dist"):
        r = m.multi_source_bfs(g, qs, algo=algo, parents=True, count_edges=True)
        assert np.array_equal(r.dist, D) and np.array_equal(r.F, ref.F)
        _valid(g, D, r.parent, algo)
        assert np.array_equal(r.edges, ref.edges)
        near = m.nearest_source(r.parent)
        for k in range(qs.K):
            assert set(near[k][near[k] >= 0].tolist()) <= set(qs.group(k).tolist())
    assert m.multi_source_bfs(g, qs, algo="bitpar", distances=True).parent is None


# ---- edge cases of the contract -------------------------------------------------------------------
def _edge_case(m):
    # 40 isolated vertices at the very end of the id range (ids >= every edge endpoint)
    base = m.Graph.uniform(3000, 9000, 11)
    deg = np.diff(base.rowptr)
    u = np.repeat(np.arange(base.n, dtype=np.int32), deg)
    keep = u < base.col
    n = base.n + 40
    g = m.Graph.from_edges(n, u[keep], base.col[keep].astype(np.int32))
    groups = [[n - 1], [n - 1, n - 2, 5], [n, n + 3, -1, 2 ** 31 - 1], [], [7, 7, 7, 7],
              [n - 40, 0], [11, 12, 11, 12, 3000]]
    groups += [[int(x)] for x in range(100, 160)]  # (two words)
    qs = m.QuerySet.from_groups(groups)
    return g, qs, _oracle("edge", g, qs)


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("algo", ["bitpar", "dist", "sweep"])
def test_edge_cases_on_device(msbfs_pkg, algo, relabel):
    import torch
    m = msbfs_pkg
    g, qs, D = _edge_case(m)
    n = g.n
    dg = _dev(g, relabel)
    with m.Solver(dg, algo, max_groups=qs.K) as s:
        r = s.parents(qs)
        E = _same(r, g, dg, D, f"{algo} relabel={relabel}")
        assert (r.parent[2] == -1).all() and (r.parent[3] == -1).all()
        assert r.parent[0][n - 1] == n - 1 and (r.parent[0] >= 0).sum() == 1
        ld = n + 7
        db = torch.full((qs.K, ld), SENTINEL, dtype=torch.int32, device="cuda:0")
        pb = torch.full((qs.K, ld), SENTINEL, dtype=torch.int32, device="cuda:0")
        r2 = s.parents(qs, dist_ptr=db.data_ptr(), parent_ptr=pb.data_ptr(), ld=ld)
        hd, hp = db.cpu().numpy(), pb.cpu().numpy()
        assert r2.parent is None and np.array_equal(r2.F, r.F)
        assert np.array_equal(hd[:, :n], D) and (hd[:, n:] == SENTINEL).all()
        assert np.array_equal(hp[:, :n], E) and (hp[:, n:] == SENTINEL).all()
        e = s.parents(m.QuerySet.from_groups([]))
        assert e.parent.shape == (0, n) and e.dist.shape == (0, n)


# ---- isolation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["bitpar", "dist"])
def test_runs_unchanged_around_parents(msbfs_pkg, algo):
    m = msbfs_pkg
    name, g = _graphs(m)[1]
    K = 200 if algo == "bitpar" else 9
    qs = m.QuerySet.random(g.n, K, 5, seed=3)
    with m.Solver(_dev(g, True), algo, max_groups=K) as s:
        a = s.run(qs, count_edges=True)
        p = s.run(qs)
        tr = [(t["level"], t["dir"], t["kind"], t["nf"]) for t in s.level_trace()]
        d = s.distances(qs)
        pa = s.parents(qs)
        b = s.run(qs, count_edges=True)
        p2 = s.run(qs)
        tr2 = [(t["level"], t["dir"], t["kind"], t["nf"]) for t in s.level_trace()]
        d2 = s.distances(qs)
        pa2 = s.parents(qs)
    assert np.array_equal(a.F, b.F) and np.array_equal(a.edges, b.edges)
    assert np.array_equal(p.F, p2.F) and np.array_equal(p.F, a.F) and tr == tr2
    assert np.array_equal(d.F, a.F) and np.array_equal(d.dist, d2.dist)
    assert np.array_equal(pa.F, a.F) and np.array_equal(pa.dist, d.dist)
    assert np.array_equal(pa.parent, pa2.parent) and np.array_equal(pa.dist, pa2.dist)
    assert a.parent is None and p.parent is None and d.parent is None and d2.parent is None


# ---- property -------------------------------------------------------------------------------------------
def _hyp_strategy():
    from hypothesis import strategies as st

    @st.composite
    def graphs_and_queries(draw):
        n = draw(st.integers(1, 60))
        m_ = draw(st.integers(0, 150))
        edges = draw(st.lists(st.tuples(st.integers(0, n - 1), st.integers(0, n - 1)),
                              min_size=m_, max_size=m_))
        K = draw(st.integers(1, 140))  # up to three 64-group words
        groups = draw(st.lists(st.lists(st.integers(-3, n + 3), max_size=6), min_size=K,
                               max_size=K))
        return n, edges, groups, draw(st.booleans()), draw(st.sampled_from([0, 1, 2]))
    return graphs_and_queries()


def test_parents_property(msbfs_pkg):
    """tiny random multigraphs (self-loops, duplicate edges, isolated vertices) and query sets
    (empty groups, out-of-range ids) through every device solver, relabelled or not"""
    from hypothesis import given, settings, HealthCheck
    from msbfs.ops.reference import bfs_dist_numpy
    m = msbfs_pkg

    @settings(max_examples=25, deadline=None, suppress_health_check=list(HealthCheck))
    @given(_hyp_strategy())
    def check(data):
        n, edges, groups, relabel, force_dir = data
        g = m.Graph.from_edges(n, np.array([e[0] for e in edges], np.int32),
                               np.array([e[1] for e in edges], np.int32))
        qs = m.QuerySet.from_groups(groups)
        D = np.stack([bfs_dist_numpy(g.n, g.rowptr, g.col, qs.group(k)) for k in range(qs.K)]
                     ).astype(np.int32)
        dg = _dev(g, relabel)
        with m.Solver(dg, "bitpar", max_groups=qs.K, force_dir=force_dir) as s:
            _same(s.parents(qs), g, dg, D, "bitpar")
        for algo in ("dist", "topdown", "sweep"):
            sub = qs.subset(np.arange(min(qs.K, 4)))
            with m.Solver(dg, algo) as s:
                _same(s.parents(sub), g, dg, D[:sub.K], algo)
        dg.close()
        _EDGESETS.clear()

    check()


# ---- native CLI -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["bitpar", "dist"])
def test_native_cli_parent_out(tmp_path, msbfs_pkg, algo):
    """the CLI relabels by degree (sorted rows, a map that depends on the graph alone): the same
    device graph built here gives oracle (a) for the reported winner"""
    m = msbfs_pkg
    cli = m.native.CLI_PATH
    if not os.path.exists(cli):
        pytest.fail("native CLI not built (make -C csrc)")
    g = m.Graph.rmat(12, 8, 3)
    qs = m.QuerySet.random(g.n, 70, 3, seed=7)
    gp, qp = str(tmp_path / "g.bin"), str(tmp_path / "q.bin")
    dp, pp = str(tmp_path / "d.bin"), str(tmp_path / "p.bin")
    g.write(gp)
    qs.write(qp)
    env = dict(os.environ, MSBFS_NO_MPI="1")
    r = subprocess.run([cli, "-g", gp, "-q", qp, "-gn", "1", "--algo", algo, "--no-cache",
                        "--parent-out", pp, "--dist-out", dp], capture_output=True, text=True,
                       env=env, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 7, r.stdout
    k = int(lines[2].split(":")[1]) - 1  # the reported winner
    ref = m.cpu_bfs(g, qs)
    assert k == m.argmin_first(ref.F) and lines[3] == f"Minimum F value: {ref.F[k]}"
    from msbfs.ops.reference import bfs_dist_numpy
    D = bfs_dist_numpy(g.n, g.rowptr, g.col, qs.group(k)).astype(np.int32)[None, :]
    assert np.array_equal(np.fromfile(dp, dtype="<i4"), D[0])
    p = np.fromfile(pp, dtype="<i4").astype(np.int32)
    _valid(g, D, p[None, :], algo)
    dg = _dev(g, True)
    assert np.array_equal(p, _expected(dg, D)[0])
