"""BFS parents on the host path: cpu_bfs(parents=True) / msbfs_cpu_run_parents against (a) the
exact first-in-row matrix worked out from the numpy distance oracle and the host CSR and (b) an
independent validity check; the numpy helpers path_to_set / nearest_source; the Python CLI's
--parent-out round trip; and the stand-alone sanitizer program of the host code."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(g, qs):
    from msbfs.ops.reference import bfs_dist_numpy
    D = np.full((qs.K, g.n), -1, dtype=np.int32)
    for k in range(qs.K):
        D[k] = bfs_dist_numpy(g.n, g.rowptr, g.col, qs.group(k))
    return D


def _expected(g, D):
    """(a): parent[k, v] = v for sources, -1 unreached, else the first entry of v's row in g at
    distance D[k, v] - 1"""
    K, n = D.shape
    P = np.full((K, n), -1, dtype=np.int32)
    deg = np.diff(g.rowptr)
    row_of = np.repeat(np.arange(n), deg)          # the vertex of every CSR entry
    pos = np.arange(len(g.col)) - g.rowptr[row_of]  # its position in the row
    for k in range(K):
        d = D[k]
        ok = (d[row_of] > 0) & (d[g.col] == d[row_of] - 1)
        first = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(first, row_of[ok], pos[ok])
        has = d > 0
        assert (first[has] < deg[has]).all()
        P[k, has] = g.col[g.rowptr[:-1][has] + first[has]]
        P[k, d == 0] = np.nonzero(d == 0)[0]
    return P


def _valid(g, D, P):
    """(b): sources are self-parents, unreached entries -1, (v, parent) an edge of g, the parent
    one level nearer"""
    K, n = D.shape
    assert P.dtype == np.int32 and P.shape == D.shape
    edges = set(zip(np.repeat(np.arange(n), np.diff(g.rowptr)).tolist(), g.col.tolist()))
    for k in range(K):
        d, p = D[k], P[k]
        src = np.nonzero(d == 0)[0]
        assert np.array_equal(p[src], src), k
        assert (p[d < 0] == -1).all(), k
        rest = np.nonzero(d > 0)[0]
        assert ((p[rest] >= 0) & (p[rest] < n)).all(), k
        assert np.array_equal(d[p[rest]], d[rest] - 1), k
        assert all((int(v), int(p[v])) in edges for v in rest), k


def _check(m, g, qs, **kw):
    r = m.cpu_bfs(g, qs, parents=True, **kw)
    D = _oracle(g, qs)
    assert r.dist.dtype == np.int32 and np.array_equal(r.dist, D)
    assert np.array_equal(r.F, np.where(D >= 0, D, 0).sum(axis=1, dtype=np.int64))
    assert np.array_equal(r.F, m.cpu_bfs(g, qs).F)
    _valid(g, D, r.parent)
    assert np.array_equal(r.parent, _expected(g, D))
    return r


def _golden(m):
    for (n, edges), groups, F, _k, _minf in CASES:
        g = m.Graph.from_edges(n, np.array([e[0] for e in edges], np.int32),
                               np.array([e[1] for e in edges], np.int32))
        yield g, m.QuerySet.from_groups(groups), F


def test_cpu_parents_golden_cases(msbfs_pkg):
    m = msbfs_pkg
    for g, qs, F in _golden(m):
        r = _check(m, g, qs)
        assert list(r.F) == F


@pytest.mark.parametrize("which", ["uniform", "grid"])
def test_cpu_parents_match_oracle(msbfs_pkg, which):
    m = msbfs_pkg
    g = m.Graph.uniform(5000, 2500, 4) if which == "uniform" else m.Graph.grid(40, 60, 0.9, 5, 2)
    _check(m, g, m.QuerySet.random(g.n, 9, 3, seed=5), threads=1)
    _check(m, g, m.QuerySet.random(g.n, 5, 3, seed=6), threads=3)


def test_cpu_parents_odd_sources(msbfs_pkg):
    """out-of-range and duplicate ids, an empty group, a group with no valid id"""
    m = msbfs_pkg
    g = m.Graph.uniform(5000, 2500, 4)
    n = g.n
    qs = m.QuerySet.from_groups([[3, 3, 3, 17, 3], [], [-1, n, n + 5, 2 ** 31 - 1],
                                 [n - 1, -7, 0, n - 1], [n, 40]])
    r = _check(m, g, qs)
    assert (r.parent[1] == -1).all() and (r.parent[2] == -1).all()
    assert r.parent[0][3] == 3 and r.parent[0][17] == 17
    assert r.parent[3][n - 1] == n - 1 and r.parent[3][0] == 0


def test_cpu_parent_is_first_in_row_not_the_discoverer(msbfs_pkg):
    """0-1, 0-2, and 3 whose row is [2, 1]: the queue discovers 3 from 1, its parent is 2"""
    m = msbfs_pkg
    g = m.Graph.from_edges(5, np.array([0, 0, 2, 1], np.int32), np.array([1, 2, 3, 3], np.int32),
                           stable=True)
    assert list(g.col[g.rowptr[3]:g.rowptr[4]]) == [2, 1]
    r = _check(m, g, m.QuerySet.from_groups([[0]]))
    assert list(r.parent[0]) == [0, 0, 0, 2, -1]


def test_plain_and_distance_results_carry_no_parents(msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.rmat(9, 8, 3)
    qs = m.QuerySet.random(g.n, 6, 2, seed=2)
    assert m.cpu_bfs(g, qs).parent is None and m.cpu_bfs(g, qs, distances=True).parent is None
    r = m.multi_source_bfs(g, qs, algo="cpu", parents=True, count_edges=True)
    ref = m.cpu_bfs(g, qs, count_edges=True)
    D = _oracle(g, qs)
    assert np.array_equal(r.dist, D) and np.array_equal(r.parent, _expected(g, D))
    assert np.array_equal(r.F, ref.F) and np.array_equal(r.edges, ref.edges)


def test_path_to_set(msbfs_pkg):
    """every hop is an edge, the path ends at a source of the group, its length is dist + 1"""
    m = msbfs_pkg
    g = m.Graph.grid(40, 60, 0.9, 5, 2)
    qs = m.QuerySet.random(g.n, 3, 3, seed=5)
    r = m.cpu_bfs(g, qs, parents=True)
    edges = set(zip(np.repeat(np.arange(g.n), np.diff(g.rowptr)).tolist(), g.col.tolist()))
    rng = np.random.default_rng(1)
    for k in range(qs.K):
        far = int(np.argmax(r.dist[k]))
        for v in [far] + rng.integers(0, g.n, 40).tolist() + qs.group(k).tolist():
            path = m.path_to_set(r.parent[k], v)
            if r.dist[k, v] < 0:
                assert path == []
                continue
            assert len(path) == r.dist[k, v] + 1 and path[0] == v
            assert path[-1] in set(qs.group(k).tolist())
            assert all((a, b) in edges for a, b in zip(path, path[1:]))
            assert [int(r.dist[k, x]) for x in path] == list(range(int(r.dist[k, v]), -1, -1))
    unreached = m.Graph.from_edges(3, np.array([0], np.int32), np.array([1], np.int32))
    p = m.cpu_bfs(unreached, m.QuerySet.from_groups([[0]]), parents=True).parent[0]
    assert m.path_to_set(p, 2) == [] and m.path_to_set(p, 1) == [1, 0]
    assert m.path_to_set(p, 0) == [0]


def test_nearest_source(msbfs_pkg):
    """the result is a valid source of the group at distance dist, by single-source BFS"""
    from msbfs.ops.reference import bfs_dist_numpy
    m = msbfs_pkg
    g = m.Graph.uniform(300, 330, 7)  # (several components: unreached vertices)
    qs = m.QuerySet.from_groups([[5, 100, 250], [7], [], [299, 299, 300, 0]])
    r = m.cpu_bfs(g, qs, parents=True)
    near = m.nearest_source(r.parent)
    assert near.dtype == np.int32 and near.shape == (qs.K, g.n)
    assert (r.dist < 0).any() and (r.dist > 2).any()
    single = {}
    for k in range(qs.K):
        valid = {int(s) for s in qs.group(k) if 0 <= s < g.n}
        assert np.array_equal(near[k] < 0, r.dist[k] < 0)
        for v in np.nonzero(r.dist[k] >= 0)[0]:
            s = int(near[k, v])
            assert s in valid
            if s not in single:
                single[s] = bfs_dist_numpy(g.n, g.rowptr, g.col, np.array([s], np.int32))
            assert single[s][v] == r.dist[k, v]
            assert m.path_to_set(r.parent[k], int(v))[-1] == s
    assert np.array_equal(m.nearest_source(r.parent[0]), near[0])  # (one row)


def _py_cli(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "msbfs"] + args, capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=300)


def test_python_cli_parent_out_round_trip(tmp_path, msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.grid(12, 17, 0.9, 3, 2)
    qs = m.QuerySet.random(g.n, 5, 2, seed=4)
    gp, qp = str(tmp_path / "g.bin"), str(tmp_path / "q.bin")
    dp, pp = str(tmp_path / "d.bin"), str(tmp_path / "p.bin")
    g.write(gp)
    qs.write(qp)
    base = ["-g", gp, "-q", qp, "-gn", "1", "--algo", "cpu"]
    plain = _py_cli(base)
    r = _py_cli(base + ["--parent-out", pp, "--dist-out", dp])
    assert r.returncode == 0 and plain.returncode == 0, r.stderr[-2000:]
    # the report is what it is without the flag (timings aside)
    assert r.stdout.splitlines()[:5] == plain.stdout.splitlines()[:5]
    assert len(r.stdout.splitlines()) == 7
    ref = m.cpu_bfs(g, qs)
    k = m.argmin_first(ref.F)
    assert r.stdout.splitlines()[2].endswith(f": {k + 1}")
    # the CLI ran on the graph file's CSR: the same host graph
    gf = m.Graph.from_file(gp)
    D = _oracle(gf, qs)
    p = np.fromfile(pp, dtype="<i4")
    assert np.array_equal(np.fromfile(dp, dtype="<i4"), D[k])
    _valid(g, D[k:k + 1], p[None, :].astype(np.int32))
    assert np.array_equal(p, _expected(gf, D[k:k + 1])[0])
    # K = 0: nothing written
    m.QuerySet.from_groups([]).write(qp)
    p0 = str(tmp_path / "p0.bin")
    r = _py_cli(base + ["--parent-out", p0])
    assert r.returncode == 0 and not os.path.exists(p0)


def test_native_cli_parent_out_cpu(tmp_path, msbfs_pkg):
    m = msbfs_pkg
    cli = m.native.CLI_PATH
    if not os.path.exists(cli):
        pytest.fail("native CLI not built (make -C csrc)")
    g = m.Graph.uniform(400, 900, 3)
    qs = m.QuerySet.random(g.n, 7, 2, seed=8)
    gp, qp, pp = str(tmp_path / "g.bin"), str(tmp_path / "q.bin"), str(tmp_path / "p.bin")
    g.write(gp)
    qs.write(qp)
    env = dict(os.environ, MSBFS_NO_MPI="1")
    base = [cli, "-g", gp, "-q", qp, "-gn", "1", "--algo", "cpu", "--no-cache"]
    plain = subprocess.run(base, capture_output=True, text=True, env=env, timeout=300)
    r = subprocess.run(base + ["--parent-out", pp], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines()[:5] == plain.stdout.splitlines()[:5]
    assert len(r.stdout.splitlines()) == 7
    k = m.argmin_first(m.cpu_bfs(g, qs).F)
    D = _oracle(g, qs)[k:k + 1]
    p = np.fromfile(pp, dtype="<i4").astype(np.int32)
    # (the native loader's row order is its own: the validity check decides)
    assert p.shape == (g.n,)
    _valid(g, D, p[None, :])


@pytest.mark.parametrize("kind", ["asan", "tsan"])
def test_parents_host_code_under_sanitizers(kind):
    """csrc/tests/parents_selftest.cpp, a stand-alone program: the CPU parent pass (threaded) and
    the staging arithmetic of the host-output device runs, ASan + UBSan and TSan"""
    san = os.path.join(ROOT, "build", "san")
    make = ["make", "-C", os.path.join(ROOT, "csrc")]
    # the one reason to skip: the host compiler cannot build and run an empty program with this
    # sanitizer. A failed build of the project's own sources fails the test.
    probe = subprocess.run(make + [f"san-probe-{kind}"], capture_output=True, text=True,
                           timeout=300)
    if probe.returncode != 0:
        pytest.skip(f"the host compiler has no {kind}: {probe.stderr[-400:]}")
    b = subprocess.run(make + [f"parents-{kind}"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["TSAN_OPTIONS"] = "halt_on_error=1"
    r = subprocess.run([os.path.join(san, f"parents_selftest_{kind}")], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "parents selftest: ok" in r.stdout
    assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr
