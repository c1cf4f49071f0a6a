"""Every kind of run (plain, edge counts, distances, parents, level profiles) interleaved on ONE
solver, for each device solver: what a distance, parents or profile run sets up must be gone in
the next run, and leaf folding of the bit-parallel solver must come back after the runs that
switch it off. Every value is held against the CPU oracle on the device graph's own download()
(internal ids), mapped through relabel_map() as test_parents_gpu.py does; exact integers."""
import numpy as np
import pytest

import profile_oracle

pytestmark = pytest.mark.gpu

K, PAD, FILL = 70, 3, 7
SOLVERS = [("bitpar", dict(tuning="leaf=1")),               # 2 words, the second one partial
           ("bitpar", dict(tuning="leaf=1", max_words=1)),  # two batches
           ("dist", {}), ("sweep", {})]

_CASE = {}


def _case(m):
    """(device graph, queries, oracle), built once: F, edges, dist, parent by user id, profile"""
    if _CASE:
        return _CASE["v"]
    g = m.DeviceGraph.rmat(11, 16, seed=1, relabel=True)
    assert g.relabelled
    h, n = g.download(), g.n
    o2n = g.relabel_map().astype(np.int64)
    n2o = np.empty(n, dtype=np.int64)
    n2o[o2n] = np.arange(n)
    leaves = np.flatnonzero(np.diff(h.rowptr) == 1)
    assert len(leaves)
    groups = np.random.RandomState(5).randint(0, n, (K, 3))
    groups[5] = [-1, n, n + 7]          # every id out of range
    groups[66, 0] = n2o[leaves[0]]      # a degree-1 source (second word / second batch)
    qs = m.QuerySet.from_groups(groups)
    # the oracle runs on the internal ids: sources mapped in, results mapped back
    ok = (groups >= 0) & (groups < n)
    qi = m.QuerySet.from_groups(np.where(ok, o2n[np.where(ok, groups, 0)], groups))
    ref = m.cpu_bfs(h, qi, count_edges=True)
    rp = m.cpu_bfs(h, qi, parents=True)
    assert np.array_equal(rp.F, ref.F)
    D = rp.dist[:, o2n]
    Pi = rp.parent[:, o2n].astype(np.int64)
    P = np.where(Pi >= 0, n2o[np.where(Pi >= 0, Pi, 0)], -1).astype(np.int32)
    prof = profile_oracle.from_distances(D)
    assert np.array_equal(prof[0], ref.F) and (D[5] == -1).all()
    for a in (D, P):
        a.setflags(write=False)
    _CASE["v"] = (g, qs, ref, D, P, prof)
    return _CASE["v"]


def _levels(s):
    return [(r["dir"], r["kind"], r["nf"], r["nf_next"]) for r in s.level_trace()]


@pytest.mark.parametrize("algo,kw", SOLVERS, ids=["bitpar", "bitpar-2batches", "dist", "sweep"])
def test_interleaved_kinds(msbfs_pkg, algo, kw):
    import torch
    m = msbfs_pkg
    g, qs, ref, D, P, prof = _case(m)
    n, ld = g.n, g.n + PAD
    bitpar = algo == "bitpar"
    with m.Solver(g, algo, max_groups=K, **kw) as s:
        plain = []

        def run_plain():
            r = s.run(qs)
            assert np.array_equal(r.F, ref.F) and r.edges is None
            plain.append((r.stats["leaf_folded"], _levels(s)))

        run_plain()                                                   # 1
        r = s.distances(qs)                                           # 2
        assert np.array_equal(r.F, ref.F) and np.array_equal(r.dist, D)
        assert r.parent is None and (not bitpar or r.stats["leaf_folded"] == 0)
        r = s.run(qs, count_edges=True)                               # 3
        assert np.array_equal(r.F, ref.F) and np.array_equal(r.edges, ref.edges)
        r = s.parents(qs)                                             # 4
        assert np.array_equal(r.F, ref.F) and np.array_equal(r.dist, D)
        assert np.array_equal(r.parent, P)
        assert not bitpar or r.stats["leaf_folded"] == 0
        profile_oracle.check(s.profile(qs, bins=8), prof, 8, "bins=8")  # 5
        run_plain()                                                   # 6
        r = s.profile(qs, bins="all")                                 # 7
        profile_oracle.check(r, prof, r.hist.shape[1], "bins=all")
        buf = torch.full((K, ld), FILL, dtype=torch.int32, device="cuda:0")
        r = s.distances(qs, out_ptr=buf.data_ptr(), ld=ld)            # 8
        hb = buf.cpu().numpy()
        assert r.dist is None and np.array_equal(r.F, ref.F)
        assert np.array_equal(hb[:, :n], D) and (hb[:, n:] == FILL).all()
        run_plain()                                                   # 9
    if bitpar:
        assert plain[0][0] > 0 and plain[1][0] == plain[0][0] and plain[2][0] == plain[0][0]
        assert len(plain[0][1]) and plain[2][1] == plain[0][1]
