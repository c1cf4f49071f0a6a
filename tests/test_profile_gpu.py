"""Level profiles (Solver.profile: reach, eccentricity, vertices per level) of the device solvers
against the CPU oracle, exact integers. The oracle is np.bincount over cpu_bfs(distances=True)
rows where the graph is small (profile_oracle.oracle) and cpu_bfs(profile=True, bins="all"),
itself checked against that in test_profile_cpu.py, where it is not.

The bit-parallel solver must run the kernels of run(): the cases go through leaf folding and its
source corrections, the fused push batches, the device-driven pull batches, tiles, lazy batches
and dskip, and compare the level trace of profile() with that of run()."""
import os
import subprocess

import numpy as np
import pytest

import block_loops as bl
from profile_oracle import check, oracle
from test_leaf_fold_gpu import (TRAP_EDGES, TRAP_GROUPS, TRAP_N, _caterpillar, _graph, _query)

pytestmark = pytest.mark.gpu


def _cpu_oracle(m, g, qs):
    r = m.cpu_bfs(g, qs, profile=True, bins="all")
    return r.F, r.reach, r.ecc, r.hist


def _profile(m, dg, qs, ora, tuning="", bins=(64,), algo="bitpar", max_groups=None, what=""):
    """profile() for every bin count of `bins` on one solver against the oracle tuple; returns
    the stats of the last run"""
    with m.Solver(dg, algo, max_groups=max_groups or qs.K,
                  tuning=tuning if algo == "bitpar" else None) as s:
        for b in bins:
            r = s.profile(qs, bins=b)
            check(r, ora, r.hist.shape[1], (what, tuning, b))
            if b == "all":
                assert r.hist.shape[1] >= int(ora[2].max()) + 2 and not r.hist[:, -1].any()
            else:
                assert r.hist.shape[1] == b
        return r.stats


# The trap graph of the leaf-fold test plus two components whose folded count of level 2 is taken
# away again by the source correction: the leaf 26 of 27, whose row is {26, 27} (a self-loop);
# the leaf 28 of 29, whose other edge to 30 is doubled. From [26] the eccentricity is 1, not 2.
TRAP2_N = TRAP_N + 5
TRAP2_EDGES = TRAP_EDGES + [(26, 27), (27, 27), (28, 29), (29, 30), (29, 30)]
TRAP2_GROUPS = [[26], [28], [26, 28], [27], [30], [26, 27]] + TRAP_GROUPS


@pytest.fixture(scope="module")
def traps(msbfs_pkg):
    m = msbfs_pkg
    g = _graph(m, TRAP2_N, TRAP2_EDGES)
    dg = g.to_device(0).relabel_by_degree()
    yield m, g, dg
    dg.close()


@pytest.mark.parametrize("K", [1, 64, 65, 1024])
def test_traps(traps, K):
    m, g, dg = traps
    qs = _query(m, TRAP2_N, TRAP2_GROUPS[:K], K)
    ora = oracle(m, g, qs)
    assert ora[2][0] == 1 and (K < 2 or ora[2][1] == 2)  # (the trap: a level-2 count of one source)
    leaves = int((np.diff(g.rowptr) == 1).sum())
    assert leaves == 20
    for leaf in (1, 0):
        st = _profile(m, dg, qs, ora, f"leaf={leaf}", bins=(1, 2, 3, 4, 64, "all"), what=K)
        with m.Solver(dg, "bitpar", max_groups=qs.K, tuning=f"leaf={leaf}") as s:
            assert st["leaf_folded"] == s.run(qs).stats["leaf_folded"] == (leaves if leaf else 0)
        for t in ("td_fused=0", "batch=1", "lazy=0", "bu_max=0"):
            _profile(m, dg, qs, ora, f"leaf={leaf},{t}", bins=(2, 64), what=K)


@pytest.mark.parametrize("K", [64, 1024])
def test_caterpillar_and_star(msbfs_pkg, K):
    """Every leaf weight class and the heavy parents (the 4096-vertex graph of the fold test)."""
    m = msbfs_pkg
    n, edges = _caterpillar(40, [0, 1, 2, 3, 17, 200, 16, 40, 5, 130])
    star0 = n
    edges += [(star0, star0 + 1 + i) for i in range(4096 - n - 1)]
    g = _graph(m, 4096, edges)
    first = [[0], [star0], [star0 + 1], [n - 1, star0 + 5], [39, 0], [star0 + 2, star0 + 3, star0]]
    qs = _query(m, 4096, first[:K], K)
    ora = oracle(m, g, qs) if K == 64 else _cpu_oracle(m, g, qs)
    with g.to_device(0).relabel_by_degree() as dg:
        for leaf in (1, 0):
            st = _profile(m, dg, qs, ora, f"leaf={leaf}", bins=(8, "all"))
            assert (st["leaf_folded"] > 0) == (leaf == 1)
        _profile(m, dg, qs, ora, "leaf=1,td_fused=0,dirs=TBBTB", bins=(64,))


@pytest.fixture(scope="module", params=["path300", "grid64"])
def deep(request, msbfs_pkg):
    """High-diameter graphs of degree <= 4: their push levels run as device-driven batches of
    fused levels (4, 8, ... 64 levels per batch, several k_level_reduce_multi launches each)."""
    m = msbfs_pkg
    if request.param == "path300":
        g = _graph(m, 300, [(i, i + 1) for i in range(299)])
    else:
        g = m.Graph.grid(64, 64)
    dg = g.to_device(0).relabel_by_degree()
    yield m, request.param, g, dg
    dg.close()


def _deep_query(m, g, K):
    """K groups of one or two sources from a pool of a few vertices (ends / corners and the
    middle): the union frontier stays a few vertices wide, so every level is a push level"""
    n = g.n
    pool = [0, 1, 2, n - 1, n - 2, n // 2] if n == 300 else [0, 63, n - 64, n - 1, n // 2 + 32]
    P = len(pool)
    gs = [[pool[k % P]] if k < P else [pool[k % P], pool[(k // P) % P]] for k in range(K)]
    return m.QuerySet.from_groups(gs)


@pytest.mark.parametrize("K", [64, 128])
def test_device_driven_push_batches(deep, K):
    m, name, g, dg = deep
    qs = _deep_query(m, g, K)
    ora = oracle(m, g, qs)
    assert int(ora[2].max()) == (299 if name == "path300" else 126)
    st = _profile(m, dg, qs, ora, bins=(16, "all"), what=name)
    assert st["td_levels"] == st["levels"] >= int(ora[2].max())  # (push levels only: batches)
    _profile(m, dg, qs, ora, "td_fused=0", bins=(16,), what=name)


def test_push_batches_one_block(msbfs_pkg):
    """S60 of the block-loop tests with one block per kernel (max_grid=1)."""
    m = msbfs_pkg
    g = bl.make_graph(m, "S60")
    qs = bl.queries(m, g.n, 64)
    ora = _cpu_oracle(m, g, qs)
    with g.to_device(0).relabel_by_degree() as dg:
        _profile(m, dg, qs, ora, "max_grid=1", bins=(16,))


@pytest.fixture(scope="module")
def rmat15(msbfs_pkg):
    m = msbfs_pkg
    dg = m.DeviceGraph.rmat(15, 16, 1, device=0)
    g = dg.download()
    dg.relabel_by_degree()
    refs = {}
    yield m, g, dg, refs
    dg.close()


def _rmat15_ref(m, g, refs, K):
    if K not in refs:
        qs = m.QuerySet.random(g.n, K, 8, 7)
        refs[K] = (qs, _cpu_oracle(m, g, qs))
    return refs[K]


@pytest.mark.parametrize("K", [64, 128, 1024])
@pytest.mark.parametrize("tuning", ["", "tiles=0,full=0,dskip=0"])
def test_pull_levels(rmat15, K, tuning):
    """Pull levels, tiles and the device-driven pull batches, leaf folding by its own decision."""
    m, g, dg, refs = rmat15
    qs, ora = _rmat15_ref(m, g, refs, K)
    st = _profile(m, dg, qs, ora, tuning, bins=(64, 3), what=K)
    assert st["bu_levels"] > 0
    assert st["leaf_folded"] == int((np.diff(g.rowptr) == 1).sum()) > 0


def _same_solver(m, dg, qs, ora):
    keys = ("dir", "kind", "nf", "nf_next")
    with m.Solver(dg, "bitpar", max_groups=qs.K) as s:
        s.prepare(qs)
        s.run(qs)  # (the batch lengths of a run follow the run before it)
        r0 = s.run(qs)
        t0 = [tuple(x[k] for k in keys) for x in s.level_trace()]
        rp = s.profile(qs)
        tp = [tuple(x[k] for k in keys) for x in s.level_trace()]
        check(rp, ora, 64)
        assert rp.stats["builds"] == 0
        assert tp == t0 and len(t0) == r0.stats["levels"] > 0
        for k in ("levels", "td_levels", "bu_levels", "batches", "leaf_folded"):
            assert rp.stats[k] == r0.stats[k], k
        r1 = s.run(qs)
        assert np.array_equal(r1.F, r0.F) and np.array_equal(rp.F, r0.F)
        assert [tuple(x[k] for k in keys) for x in s.level_trace()] == t0


def test_same_solver_as_run_rmat(rmat15):
    m, g, dg, refs = rmat15
    _same_solver(m, dg, *_rmat15_ref(m, g, refs, 1024))


def test_same_solver_as_run_grid(msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.grid(64, 64)
    qs = _deep_query(m, g, 64)
    with g.to_device(0).relabel_by_degree() as dg:
        _same_solver(m, dg, qs, oracle(m, g, qs))


@pytest.mark.parametrize("algo", ["dist", "topdown", "sweep", "auto"])
def test_every_algorithm(traps, algo):
    m, g, dg = traps
    qs = _query(m, TRAP2_N, TRAP2_GROUPS, len(TRAP2_GROUPS))
    _profile(m, dg, qs, oracle(m, g, qs), bins=(1, 2, 5, "all"), algo=algo, what=algo)
    g12 = m.Graph.rmat(12, 16, 1)
    q12 = m.QuerySet.random(g12.n, 16, 4, 7)
    ora = oracle(m, g12, q12)
    for relabel in (False, True):
        with g12.to_device(0) as d12:
            if relabel:
                d12.relabel_by_degree()
            _profile(m, d12, q12, ora, bins=(4, 64), algo=algo, what=(algo, relabel))


def test_two_passes(msbfs_pkg):
    """K = 2048 groups on a solver of 1024: two passes, each with its own counts."""
    m = msbfs_pkg
    g = m.Graph.rmat(12, 16, 1)
    qs = m.QuerySet.random(g.n, 2048, 3, 11)
    ora = _cpu_oracle(m, g, qs)
    with g.to_device(0).relabel_by_degree() as dg:
        st = _profile(m, dg, qs, ora, bins=(64, 2), max_groups=1024)
        assert st["batches"] == 2
        r = m.multi_source_bfs(dg, qs, algo="bitpar", profile=True, bins=5)
        check(r, ora, 5)


def test_cli_profile_out(tmp_path, msbfs_pkg):
    m = msbfs_pkg
    cli = m.native.CLI_PATH
    if not os.path.exists(cli):
        pytest.skip("native CLI not built")
    out, dout = str(tmp_path / "p.txt"), str(tmp_path / "d.bin")
    r = subprocess.run([cli, "--gen", "rmat:12:16:1", "--qgen", "100:4:7", "-gn", "1", "--algo",
                        "bitpar", "--profile-out", out, "--dist-out", dout],
                       capture_output=True, text=True, env=dict(os.environ, MSBFS_NO_MPI="1"),
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.splitlines()) == 7
    g = m.Graph.rmat(12, 16, 1)
    F, reach, ecc, H = oracle(m, g, m.QuerySet.random(g.n, 100, 4, 7))
    k = m.argmin_first(F)
    e = int(ecc[k])
    with open(out) as f:
        text = f.read()
    assert text.endswith("\n") and text.count("\n") == 1
    assert [int(x) for x in text.split()] == [k, int(reach[k]), e, int(F[k])] + \
        [int(x) for x in H[k, :e + 1]]
    assert (np.fromfile(dout, "<i4") >= 0).sum() == reach[k]
