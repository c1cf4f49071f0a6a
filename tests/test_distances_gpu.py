"""Per-vertex distances from every device solver: the whole K x n matrix against the numpy oracle
(exactly) plus F, through Solver.distances / msbfs_solver_run_dist(_host). The bit-parallel
solver records the level of every new (vertex, group) bit at three sites (host-driven push
level, device-driven push batch, pull level); the cases below reach each of them, every word
layout, several passes, relabelled graphs and the edge cases of the contract."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 123456789
_ORACLE = {}


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


def _same(r, D, what=""):
    assert r.dist is not None and r.dist.dtype == np.int32 and r.dist.shape == D.shape, what
    if not np.array_equal(r.dist, D):
        k, v = np.argwhere(r.dist != D)[0]
        raise AssertionError(f"{what}: dist[{k}, {v}] = {r.dist[k, v]}, oracle {D[k, v]} "
                             f"({int((r.dist != D).sum())} entries differ)")
    assert np.array_equal(r.F, _F_of(D)), what


def _dev(g, relabel=False):
    dg = g.to_device(0)
    if relabel:  # degree-descending internal ids; queries and distances keep the original ones
        dg.relabel_by_degree()
        assert dg.relabelled
    return dg


def _graphs(m):
    # the first four graphs of test_gpu_kernels._graphs
    return [("rmat10", m.Graph.rmat(10, 16, 3)), ("rmat12", m.Graph.rmat(12, 8, 5)),
            ("uniform", m.Graph.uniform(3000, 9000, 11)), ("grid", m.Graph.grid(40, 60, 0.9, 5, 2))]


# ---- bit-parallel: word layouts, batch offsets, passes ------------------------------------------
def _rmat11(m):
    g = m.Graph.rmat(11, 16, 9)
    qs = m.QuerySet.random(g.n, 1024, 2, seed=77)
    return g, qs, _oracle("rmat11", g, qs)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130, 300, 1024])
def test_bitpar_word_layouts(msbfs_pkg, K):
    m = msbfs_pkg
    g, qs, D = _rmat11(m)
    sub = qs.subset(np.arange(K))
    with m.Solver(g.to_device(0), "bitpar", max_groups=K) as s:
        _same(s.distances(sub), D[:K], f"K={K}")


def test_bitpar_several_passes(msbfs_pkg):
    """K = 300 over passes of 128 groups: k0 > 0 and a partial last pass (one word)"""
    m = msbfs_pkg
    g, qs, D = _rmat11(m)
    sub = qs.subset(np.arange(300))
    with m.Solver(g.to_device(0), "bitpar", max_groups=128) as s:
        r = s.distances(sub)
        assert r.stats["batches"] == 3
        _same(r, D[:300], "host output")
        import torch
        buf = torch.full((300, g.n), SENTINEL, dtype=torch.int32, device="cuda:0")
        r2 = s.distances(sub, out_ptr=buf.data_ptr())
        assert r2.dist is None and np.array_equal(r2.F, r.F)
        assert np.array_equal(buf.cpu().numpy(), D[:300])


# ---- bit-parallel: the three recording sites ----------------------------------------------------
@pytest.mark.parametrize("force_dir,wide", [(1, 64), (2, 4), (0, 1)])
def test_bitpar_recording_sites(msbfs_pkg, force_dir, wide):
    """push only / pull with hub chunks / mixed"""
    m = msbfs_pkg
    for name, g in _graphs(m):
        qs = m.QuerySet.random(g.n, 200, 5, seed=3)
        D = _oracle(("sites", name), g, qs)
        with m.Solver(g.to_device(0), "bitpar", max_groups=qs.K, force_dir=force_dir,
                      wide_degree=wide) as s:
            _same(s.distances(qs), D, f"{name} force_dir={force_dir} wide={wide}")
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
    """A road-like grid (max degree 4): the push levels run in device-driven batches, where the
    level number is fixed at enqueue time and a closed level must write nothing. With default
    options the distance run's first batch stops for a pull after two levels (its later levels
    are closed) and the remaining ~90 levels pull; push-only (force_dir = 1) runs all 93 levels
    in batches of 4, 8, 16, 32 and 64, crossing every batch boundary."""
    m = msbfs_pkg
    g = m.Graph.grid(40, 60, 0.9, 0, 2)
    qs = m.QuerySet.random(g.n, 70, 2, seed=12)
    D = _oracle("gridbatch", g, qs)
    assert int(D.max()) > 64
    with m.Solver(g.to_device(0), "bitpar", max_groups=qs.K, force_dir=force_dir) as s:
        _same(s.distances(qs), D, "grid")
        tr = s.level_trace()
    dirs = "".join(t["dir"] for t in tr)
    runs = _push_batches(tr)
    assert len(tr) >= int(D.max()) and dirs[0] == "T"
    assert runs and max(runs) <= 64, (dirs, runs)
    if force_dir == 1:
        assert set(dirs) == {"T"} and len(runs) >= 3 and sum(runs) >= 64, (dirs, runs)


# ---- relabelled graphs ----------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["bitpar", "dist", "topdown", "sweep"])
def test_relabelled_graph_original_ids(msbfs_pkg, algo):
    m = msbfs_pkg
    for name, g in _graphs(m)[:3]:
        K = 130 if algo == "bitpar" else 9
        qs = m.QuerySet.random(g.n, K, 3, seed=21)
        D = _oracle(("relabel", name, K), g, qs)
        with m.Solver(_dev(g, True), algo, max_groups=K) as s:
            _same(s.distances(qs), D, f"{name} {algo} relabelled")
        with m.Solver(g.to_device(0), algo, max_groups=K) as s:
            _same(s.distances(qs), D, f"{name} {algo}")


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
    assert (D[2] == -1).all() and (D[3] == -1).all() and D[0][n - 1] == 0 and (D[0] >= 0).sum() == 1
    dg = _dev(g, relabel)
    with m.Solver(dg, algo, max_groups=qs.K) as s:
        r = s.distances(qs)
        _same(r, D, f"{algo} relabel={relabel}")
        # ld = n + 7, device output: rows written, padding untouched, equal to the host path
        ld = n + 7
        buf = torch.full((qs.K, ld), SENTINEL, dtype=torch.int32, device="cuda:0")
        r2 = s.distances(qs, out_ptr=buf.data_ptr(), ld=ld)
        h = buf.cpu().numpy()
        assert r2.dist is None and np.array_equal(r2.F, r.F)
        assert np.array_equal(h[:, :n], r.dist) and (h[:, n:] == SENTINEL).all()
        # the host path with a padded array
        out = np.full((qs.K, ld), SENTINEL, dtype=np.int32)
        r3 = s.distances(qs, out=out)
        assert np.array_equal(out[:, :n], D) and (out[:, n:] == SENTINEL).all()
        assert np.shares_memory(r3.dist, out)
        with pytest.raises(ValueError):
            s.distances(qs, out_ptr=buf.data_ptr(), ld=n - 1)
        assert s.distances(m.QuerySet.from_groups([])).dist.shape == (0, n)


# ---- per-group solvers ------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["dist", "topdown", "sweep"])
def test_per_group_solvers(msbfs_pkg, algo):
    m = msbfs_pkg
    for name, g in _graphs(m):
        qs = m.QuerySet.random(g.n, 9, 3, seed=len(name))
        D = _oracle(("pergroup", name), g, qs)
        for relabel in (False, True):
            with m.Solver(_dev(g, relabel), algo) as s:
                _same(s.distances(qs), D, f"{name} {algo}")
                # a second call on the same solver: the lazy reset between groups and calls
                _same(s.distances(qs.subset(np.arange(8, -1, -1))), D[::-1], f"{name} {algo} again")


def test_multi_source_bfs_distances(msbfs_pkg):
    m = msbfs_pkg
    name, g = _graphs(m)[0]
    qs = m.QuerySet.random(g.n, 9, 3, seed=len(name))
    D = _oracle(("pergroup", name), g, qs)
    ref = m.cpu_bfs(g, qs, count_edges=True)
    for algo in ("auto", "bitpar", "dist"):
        r = m.multi_source_bfs(g, qs, algo=algo, distances=True, count_edges=True)
        _same(r, D, algo)
        assert np.array_equal(r.edges, ref.edges)


# ---- isolation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["bitpar", "dist"])
def test_run_unchanged_around_distances(msbfs_pkg, algo):
    m = msbfs_pkg
    name, g = _graphs(m)[1]
    K = 200 if algo == "bitpar" else 9
    qs = m.QuerySet.random(g.n, K, 5, seed=3)
    with m.Solver(_dev(g, True), algo, max_groups=K) as s:
        a = s.run(qs, count_edges=True)
        p = s.run(qs)
        tr = [(t["level"], t["dir"], t["kind"], t["nf"]) for t in s.level_trace()]
        d = s.distances(qs)
        b = s.run(qs, count_edges=True)
        p2 = s.run(qs)
        tr2 = [(t["level"], t["dir"], t["kind"], t["nf"]) for t in s.level_trace()]
        d2 = s.distances(qs)
    assert np.array_equal(a.F, b.F) and np.array_equal(a.edges, b.edges)
    assert np.array_equal(p.F, p2.F) and np.array_equal(p.F, a.F) and tr == tr2
    assert np.array_equal(d.F, a.F) and np.array_equal(d.dist, d2.dist)
    assert a.dist is None and p.dist is None


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


def test_distances_property(msbfs_pkg):
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
            _same(s.distances(qs), D, "bitpar")
        for algo in ("dist", "topdown", "sweep"):
            sub = qs.subset(np.arange(min(qs.K, 4)))
            with m.Solver(dg, algo) as s:
                _same(s.distances(sub), D[:sub.K], algo)
        dg.close()

    check()


# ---- native CLI -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["bitpar", "dist"])
def test_native_cli_dist_out(tmp_path, msbfs_pkg, algo):
    m = msbfs_pkg
    cli = m.native.CLI_PATH
    if not os.path.exists(cli):
        pytest.fail("native CLI not built (make -C csrc)")
    g = m.Graph.rmat(12, 8, 3)
    qs = m.QuerySet.random(g.n, 70, 3, seed=7)
    gp, qp, dp = str(tmp_path / "g.bin"), str(tmp_path / "q.bin"), str(tmp_path / "d.bin")
    g.write(gp)
    qs.write(qp)
    env = dict(os.environ, MSBFS_NO_MPI="1")
    r = subprocess.run([cli, "-g", gp, "-q", qp, "-gn", "1", "--algo", algo, "--no-cache",
                        "--dist-out", dp], capture_output=True, text=True, env=env, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 7, r.stdout
    k = int(lines[2].split(":")[1]) - 1  # the reported winner
    ref = m.cpu_bfs(g, qs)
    assert k == m.argmin_first(ref.F) and lines[3] == f"Minimum F value: {ref.F[k]}"
    from msbfs.ops.reference import bfs_dist_numpy
    d = np.fromfile(dp, dtype="<i4")
    assert np.array_equal(d, bfs_dist_numpy(g.n, g.rowptr, g.col, qs.group(k)))
