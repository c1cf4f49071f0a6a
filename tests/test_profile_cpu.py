"""Level profiles (reach, eccentricity, vertices per level) on the CPU path: cpu_bfs(profile=True)
and msbfs_cpu_run_profile against np.bincount over the rows of cpu_bfs(distances=True), exact
integers; the helpers harmonic / within; the argument checks; --profile-out of both CLIs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from profile_oracle import check, fold, oracle
from test_leaf_fold_gpu import TRAP_EDGES, TRAP_GROUPS, TRAP_N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph(m, n, edges):
    e = np.array(edges, np.int32).reshape(-1, 2)
    return m.Graph.from_edges(n, e[:, 0], e[:, 1])


def _cases(m):
    yield "trap", _graph(m, TRAP_N, TRAP_EDGES), m.QuerySet.from_groups(TRAP_GROUPS)
    path = _graph(m, 300, [(i, i + 1) for i in range(299)])
    yield "path", path, m.QuerySet.from_groups([[0], [299], [150], [0, 299], [7, 7, 200], [120]])
    g = m.Graph.grid(48, 48, keep=0.6)
    yield "grid", g, m.QuerySet.random(g.n, 20, 3, 5)
    g = m.Graph.rmat(12, 16, 1)
    yield "rmat12", g, m.QuerySet.random(g.n, 40, 4, 7)


@pytest.fixture(scope="module", params=["trap", "path", "grid", "rmat12"])
def case(request, msbfs_pkg):
    for name, g, qs in _cases(msbfs_pkg):
        if name == request.param:
            return name, g, qs, oracle(msbfs_pkg, g, qs)


def test_cpu_profile_matches_bincount(msbfs_pkg, case):
    m = msbfs_pkg
    name, g, qs, ora = case
    top = int(ora[2].max())
    for nbins in sorted({1, 2, max(top, 1), top + 1, top + 2}):
        check(m.cpu_bfs(g, qs, profile=True, bins=nbins), ora, nbins, (name, nbins))
    r = m.cpu_bfs(g, qs, profile=True, bins="all", threads=3)
    assert r.hist.shape[1] >= top + 2 and not r.hist[:, -1].any()
    check(r, ora, r.hist.shape[1], (name, "all"))
    assert r.dist is None and r.parent is None
    # ... and through the one-shot wrapper
    r2 = m.multi_source_bfs(g, qs, algo="cpu", profile=True, bins=top + 2)
    assert np.array_equal(r2.hist, fold(ora[3], top + 2)) and np.array_equal(r2.ecc, ora[2])


def _raw(m, g, qs, F, reach, ecc, hist, nbins, ld, threads=2):
    p = m.native.ptr
    return m.native.lib().msbfs_cpu_run_profile(
        g.n, p(g.rowptr, C.c_int64), p(g.col, C.c_int32), qs.K, p(qs.off, C.c_int64),
        p(qs.ids, C.c_int32), p(F, C.c_int64),
        None if reach is None else p(reach, C.c_int64), None if ecc is None else p(ecc, C.c_int32),
        None if hist is None else p(hist, C.c_int64), nbins, ld, threads)


def test_padding_survives_and_outputs_are_nullable(msbfs_pkg, case):
    m = msbfs_pkg
    name, g, qs, ora = case
    K, nbins, ld = qs.K, 5, 9
    F = np.zeros(K, np.int64)
    reach = np.zeros(K, np.int64)
    ecc = np.zeros(K, np.int32)
    hist = np.full((K, ld), -77, np.int64)
    assert _raw(m, g, qs, F, reach, ecc, hist, nbins, ld) == 0
    assert (hist[:, nbins:] == -77).all()
    assert np.array_equal(hist[:, :nbins], fold(ora[3], nbins))
    assert np.array_equal(F, ora[0]) and np.array_equal(reach, ora[1]) and np.array_equal(ecc, ora[2])
    # each output alone
    F2 = np.zeros(K, np.int64)
    assert _raw(m, g, qs, F2, None, None, None, 1, 0) == 0 and np.array_equal(F2, ora[0])
    e2 = np.zeros(K, np.int32)
    assert _raw(m, g, qs, F2, None, e2, None, 1, 0) == 0 and np.array_equal(e2, ora[2])
    r2 = np.zeros(K, np.int64)
    assert _raw(m, g, qs, F2, r2, None, None, 3, 0) == 0 and np.array_equal(r2, ora[1])


def test_empty_out_of_range_and_duplicate_sources(msbfs_pkg):
    m = msbfs_pkg
    g = _graph(m, 6, [(0, 1), (1, 2), (2, 3), (4, 4)])
    qs = m.QuerySet.from_groups([[], [-1, 6, 1000], [0, 0, 0], [0, 3, 3, -5, 0], [5], [4], [1, 9]])
    ora = oracle(m, g, qs)
    r = m.cpu_bfs(g, qs, profile=True, bins=6)
    check(r, ora, 6)
    assert list(r.reach[:2]) == [0, 0] and list(r.ecc[:2]) == [-1, -1] and not r.hist[:2].any()
    assert list(r.hist[2]) == [1, 1, 1, 1, 0, 0] and r.ecc[2] == 3   # duplicates count once
    assert list(r.hist[3]) == [2, 2, 0, 0, 0, 0] and r.reach[3] == 4
    assert list(r.hist[4][:2]) == [1, 0] and r.ecc[4] == 0 and r.reach[4] == 1  # isolated
    assert r.ecc[5] == 0 and r.reach[5] == 1                                   # self-loop only
    assert list(r.hist[6]) == [1, 2, 1, 0, 0, 0]
    assert m.cpu_bfs(g, m.QuerySet.from_groups([]), profile=True).hist.shape == (0, 64)


def test_harmonic_and_within_on_a_path(msbfs_pkg):
    m = msbfs_pkg
    g = _graph(m, 5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    r = m.cpu_bfs(g, m.QuerySet.from_groups([[0], [2], [9]]), profile=True, bins=8)
    assert [list(h[:5]) for h in r.hist] == [[1, 1, 1, 1, 1], [1, 2, 2, 0, 0], [0, 0, 0, 0, 0]]
    assert np.allclose(m.harmonic(r.hist), [1 + 1 / 2 + 1 / 3 + 1 / 4, 2 + 2 / 2, 0.0], rtol=0,
                       atol=1e-15)
    assert m.harmonic(r.hist).dtype == np.float64 and m.harmonic(r.hist[1]) == 3.0
    assert list(m.within(r.hist, 0)) == [1, 1, 0] and list(m.within(r.hist, 1)) == [2, 3, 0]
    assert list(m.within(r.hist, 2)) == [3, 5, 0] and list(m.within(r.hist, 100)) == [5, 5, 0]
    assert list(m.within(r.hist, -1)) == [0, 0, 0] and m.within(r.hist[0], 3) == 4
    # a tail that holds vertices has no single distance
    r3 = m.cpu_bfs(g, m.QuerySet.from_groups([[0]]), profile=True, bins=3)
    assert list(r3.hist[0]) == [1, 1, 3]
    with pytest.raises(ValueError):
        m.harmonic(r3.hist)
    with pytest.raises(ValueError):
        m.within(r3.hist, 2)
    assert list(m.within(r3.hist, 1)) == [2]
    assert list(m.harmonic(np.array([[7]]))) == [0.0]  # (one bin: nothing at a known distance >= 1)


def test_error_paths(msbfs_pkg):
    m = msbfs_pkg
    g = _graph(m, 4, [(0, 1), (1, 2)])
    qs = m.QuerySet.from_groups([[0], [3]])
    F = np.zeros(2, np.int64)
    hist = np.zeros((2, 4), np.int64)
    err = lambda: m.native.lib().msbfs_last_error().decode()  # noqa: E731
    assert _raw(m, g, qs, F, None, None, hist, 0, 4) != 0 and "nbins" in err()
    assert _raw(m, g, qs, F, None, None, hist, -3, 4) != 0 and "nbins" in err()
    assert _raw(m, g, qs, F, None, None, hist, 5, 4) != 0 and "ld" in err()
    assert _raw(m, g, qs, F, None, None, None, 5, 0) == 0   # (no hist: ld is not looked at)
    assert not hist.any()
    for bad in (0, -1, "every"):
        with pytest.raises(ValueError):
            m.cpu_bfs(g, qs, profile=True, bins=bad)
    with pytest.raises(ValueError):
        m.cpu_bfs(g, qs, profile=True, distances=True)
    with pytest.raises(ValueError):
        m.multi_source_bfs(g, qs, algo="cpu", profile=True, parents=True)


def _line(path):
    with open(path) as f:
        text = f.read()
    assert text.endswith("\n") and text.count("\n") == 1
    return [int(x) for x in text.split()]


def _expect(m, g, qs):
    F, reach, ecc, H = oracle(m, g, qs)
    k = m.argmin_first(F)
    e = int(ecc[k])
    return [k, int(reach[k]), e, int(F[k])] + [int(x) for x in H[k, :e + 1]]


def test_cli_profile_out_cpu(tmp_path, msbfs_pkg):
    m = msbfs_pkg
    cli = m.native.CLI_PATH
    if not os.path.exists(cli):
        pytest.skip("native CLI not built")
    g = m.Graph.rmat(9, 8, 2)
    want = _expect(m, g, m.QuerySet.random(g.n, 20, 3, 5))
    env = dict(os.environ, MSBFS_NO_MPI="1")
    out, dout = str(tmp_path / "p.txt"), str(tmp_path / "d.bin")
    r = subprocess.run([cli, "--gen", "rmat:9:8:2", "--qgen", "20:3:5", "-gn", "1", "--algo", "cpu",
                        "--profile-out", out, "--dist-out", dout],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.splitlines()) == 7  # (the report is unchanged)
    assert _line(out) == want
    d = np.fromfile(dout, "<i4")
    assert (d >= 0).sum() == want[1] and d.max() == want[2]


def test_python_cli_profile_out_cpu(tmp_path, msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.rmat(9, 8, 2)
    qs = m.QuerySet.random(g.n, 20, 3, 5)
    gp, qp, out = str(tmp_path / "g.bin"), str(tmp_path / "q.bin"), str(tmp_path / "p.txt")
    g.write(gp)
    qs.write(qp)
    r = subprocess.run([sys.executable, "-m", "msbfs", "-g", gp, "-q", qp, "-gn", "1", "--algo",
                        "cpu", "--profile-out", out], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert _line(out) == _expect(m, g, qs)
