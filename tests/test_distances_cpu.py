"""Per-vertex distances on the host path: cpu_bfs(distances=True) / msbfs_cpu_run_dist against the
numpy oracle of the reference semantics (main.cu:40-73: 0 for valid sources, out-of-range ids
dropped, -1 for unreached vertices), and the Python CLI's --dist-out round trip."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(g, qs):
    from msbfs.ops.reference import bfs_dist_numpy
    D = np.full((qs.K, g.n), -1, dtype=np.int64)
    for k in range(qs.K):
        D[k] = bfs_dist_numpy(g.n, g.rowptr, g.col, qs.group(k))
    return D


def _check(m, g, qs, **kw):
    r = m.cpu_bfs(g, qs, distances=True, **kw)
    assert r.dist.dtype == np.int32 and r.dist.shape == (qs.K, g.n)
    D = _oracle(g, qs)
    for k in range(qs.K):
        assert np.array_equal(r.dist[k], D[k]), k
        assert int(r.dist[k][r.dist[k] >= 0].sum()) == int(r.F[k]), k
    assert np.array_equal(r.F, m.cpu_bfs(g, qs).F)
    return r


def _golden(m):
    for (n, edges), groups, F, _k, _minf in CASES:
        g = m.Graph.from_edges(n, np.array([e[0] for e in edges], np.int32),
                               np.array([e[1] for e in edges], np.int32))
        yield g, m.QuerySet.from_groups(groups), F


def test_cpu_distances_golden_cases(msbfs_pkg):
    m = msbfs_pkg
    for g, qs, F in _golden(m):
        r = _check(m, g, qs)
        assert list(r.F) == F


@pytest.mark.parametrize("which", ["uniform", "grid"])
def test_cpu_distances_match_oracle(msbfs_pkg, which):
    m = msbfs_pkg
    g = m.Graph.uniform(5000, 2500, 4) if which == "uniform" else m.Graph.grid(40, 60, 0.9, 5, 2)
    _check(m, g, m.QuerySet.random(g.n, 9, 3, seed=5))
    _check(m, g, m.QuerySet.random(g.n, 5, 3, seed=6), threads=3)


def test_cpu_distances_odd_sources(msbfs_pkg):
    """out-of-range and duplicate ids, an empty group, a group with no valid id"""
    m = msbfs_pkg
    g = m.Graph.uniform(5000, 2500, 4)
    n = g.n
    qs = m.QuerySet.from_groups([[3, 3, 3, 17, 3], [], [-1, n, n + 5, 2 ** 31 - 1],
                                 [n - 1, -7, 0, n - 1], [n, 40]])
    r = _check(m, g, qs)
    assert (r.dist[1] == -1).all() and (r.dist[2] == -1).all()
    assert r.F[1] == 0 and r.F[2] == 0
    assert r.dist[0][3] == 0 and r.dist[0][17] == 0
    assert r.dist[3][n - 1] == 0 and r.dist[3][0] == 0


def test_cpu_distances_padding_survives(msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.grid(40, 60, 0.9, 5, 2)
    qs = m.QuerySet.random(g.n, 4, 2, seed=9)
    out = np.full((qs.K, g.n + 7), 123456789, dtype=np.int32)
    r = m.cpu_bfs(g, qs, distances=True, out=out)
    assert np.array_equal(out[:, :g.n], _oracle(g, qs))
    assert (out[:, g.n:] == 123456789).all()
    assert r.dist.base is out or r.dist.base is out.base or np.shares_memory(r.dist, out)
    with pytest.raises(ValueError):
        m.cpu_bfs(g, qs, distances=True, out=np.zeros((qs.K, g.n - 1), np.int32))


def test_multi_source_bfs_cpu_distances(msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.rmat(9, 8, 3)
    qs = m.QuerySet.random(g.n, 6, 2, seed=2)
    r = m.multi_source_bfs(g, qs, algo="cpu", distances=True, count_edges=True)
    ref = m.cpu_bfs(g, qs, count_edges=True)
    assert np.array_equal(r.dist, _oracle(g, qs))
    assert np.array_equal(r.F, ref.F) and np.array_equal(r.edges, ref.edges)
    assert m.cpu_bfs(g, qs).dist is None  # (the plain result carries none)


def _py_cli(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "msbfs"] + args, capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=300)


def test_python_cli_dist_out_round_trip(tmp_path, msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.grid(12, 17, 0.9, 3, 2)
    qs = m.QuerySet.random(g.n, 5, 2, seed=4)
    gp, qp, dp = str(tmp_path / "g.bin"), str(tmp_path / "q.bin"), str(tmp_path / "d.bin")
    g.write(gp)
    qs.write(qp)
    base = ["-g", gp, "-q", qp, "-gn", "1", "--algo", "cpu"]
    plain = _py_cli(base)
    r = _py_cli(base + ["--dist-out", dp])
    assert r.returncode == 0 and plain.returncode == 0, r.stderr[-2000:]
    # the report is what it is without the flag (timings aside)
    assert r.stdout.splitlines()[:5] == plain.stdout.splitlines()[:5]
    assert len(r.stdout.splitlines()) == 7
    ref = m.cpu_bfs(g, qs)
    k = m.argmin_first(ref.F)
    assert r.stdout.splitlines()[2].endswith(f": {k + 1}")
    d = np.fromfile(dp, dtype="<i4")
    assert np.array_equal(d, _oracle(g, qs)[k])
    assert int(d[d >= 0].sum()) == int(ref.F[k])
    assert not os.path.exists(str(tmp_path / "none.bin"))


def test_python_cli_dist_out_without_groups(tmp_path, msbfs_pkg):
    """K = 0: the flag writes nothing"""
    m = msbfs_pkg
    g = m.Graph.grid(5, 5, 1.0, 0, 1)
    gp, qp, dp = str(tmp_path / "g.bin"), str(tmp_path / "q.bin"), str(tmp_path / "d.bin")
    g.write(gp)
    m.QuerySet.from_groups([]).write(qp)
    r = _py_cli(["-g", gp, "-q", qp, "-gn", "1", "--algo", "cpu", "--dist-out", dp])
    assert r.returncode == 0, r.stderr[-2000:]
    assert not os.path.exists(dp)


def test_native_cli_dist_out_cpu(tmp_path, msbfs_pkg):
    m = msbfs_pkg
    cli = m.native.CLI_PATH
    if not os.path.exists(cli):
        pytest.skip("native CLI not built")
    g = m.Graph.uniform(400, 900, 3)
    qs = m.QuerySet.random(g.n, 7, 2, seed=8)
    gp, qp, dp = str(tmp_path / "g.bin"), str(tmp_path / "q.bin"), str(tmp_path / "d.bin")
    g.write(gp)
    qs.write(qp)
    env = dict(os.environ, MSBFS_NO_MPI="1")
    r = subprocess.run([cli, "-g", gp, "-q", qp, "-gn", "1", "--algo", "cpu", "--no-cache",
                        "--dist-out", dp], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == 7
    ref = m.cpu_bfs(g, qs)
    k = m.argmin_first(ref.F)
    d = np.fromfile(dp, dtype="<i4")
    assert np.array_equal(d, _oracle(g, qs)[k])
    # K = 0 writes nothing
    m.QuerySet.from_groups([]).write(qp)
    dp0 = str(tmp_path / "d0.bin")
    r = subprocess.run([cli, "-g", gp, "-q", qp, "-gn", "1", "--algo", "cpu", "--no-cache",
                        "--dist-out", dp0], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not os.path.exists(dp0)
