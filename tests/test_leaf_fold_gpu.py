"""Leaf folding of the bit-parallel solver (tuning key leaf; csrc/src/kernels/bitpar/leaf.hpp):
the degree-1 vertices of a degree-relabelled graph stay out of the traversal and are counted
through their only neighbour. Every case: F with leaf=1 equals F with leaf=0 and the CPU oracle,
exact integers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [1, 64, 65, 1024]  # one, one, two and sixteen words per vertex


def _device(m, g):
    return g.to_device(0).relabel_by_degree()


def _check(m, g, qs, tuning="", dg=None, expect_folded=None, ref=None):
    """F of leaf=1 and leaf=0 (plus `tuning`) against the CPU oracle; returns the folded result."""
    ref = m.cpu_bfs(g, qs) if ref is None else ref
    own = dg is None
    dg = _device(m, g) if own else dg
    try:
        out = []
        for leaf in (1, 0):
            t = f"leaf={leaf}" + ("," + tuning if tuning else "")
            with m.Solver(dg, "bitpar", max_groups=qs.K, tuning=t) as s:
                r = s.run(qs)
            assert np.array_equal(r.F, ref.F), (t, np.flatnonzero(r.F != ref.F)[:8],
                                                r.F[r.F != ref.F][:8], ref.F[r.F != ref.F][:8])
            assert len(r.stats) and (leaf == 1 or r.stats["leaf_folded"] == 0)
            out.append(r)
        if expect_folded is not None:
            assert out[0].stats["leaf_folded"] == expect_folded
        return out[0]
    finally:
        if own:
            dg.close()


def _graph(m, n, edges):
    e = np.array(edges, np.int32).reshape(-1, 2)
    return m.Graph.from_edges(n, e[:, 0], e[:, 1])


def _query(m, n, first, K):
    """`first`, then one- and two-source groups over the vertices in turn: K groups in all."""
    gs = [list(x) for x in first]
    k = 0
    while len(gs) < K:
        gs.append([k % n, (3 * k + 1) % n] if k % 3 else [k % n])
        k += 1
    return m.QuerySet.from_groups(gs[:K])


# A small graph with every trap in it:
#   hub 0 with the leaves 1-5 and the core neighbours 6, 7; hub 6 with the leaves 8, 9; 7 - 10 -
#   11 a path whose end 11 is a leaf one level deeper than anything else; 12 = 13 a two-vertex
#   component; 14 with a doubled edge to 0 (degree 2: not folded); 15 with a self-loop only;
#   16 isolated; 17 - 18 another two-vertex component; star centre 19 with the leaves 20-25 only.
TRAP_N = 26
TRAP_EDGES = ([(0, v) for v in (1, 2, 3, 4, 5, 6, 7)] + [(6, 8), (6, 9), (7, 10), (10, 11),
              (12, 13), (0, 14), (0, 14), (15, 15), (17, 18)] + [(19, v) for v in range(20, 26)])
TRAP_GROUPS = [
    [1],            # a leaf source only
    [1, 0],         # a leaf source whose parent is a source too
    [2, 2],         # the same leaf twice in one group
    [2],            # ... and one leaf in several groups
    [2, 8],
    [12],           # two-vertex component, one end
    [12, 13],       # ... both ends
    [14],           # the doubled edge
    [15],           # self-loop only
    [16],           # isolated
    [20, 21],       # all sources leaves (of a star whose whole row is leaves)
    [19],           # the star's centre
    [11],           # a leaf at the deep end
    [9, 11, 3],
    [16, 15],       # nothing but isolated and self-loop
    [17, 18, 12],
    [0],
    [6, 7],
]


@pytest.mark.parametrize("K", KS)
def test_traps(msbfs_pkg, K):
    m = msbfs_pkg
    g = _graph(m, TRAP_N, TRAP_EDGES)
    qs = _query(m, TRAP_N, TRAP_GROUPS[:K], K)
    deg = np.diff(g.rowptr)
    r = _check(m, g, qs, expect_folded=int((deg == 1).sum()))
    assert r.stats["leaf_folded"] == 18
    # the same with host-driven one-kernel levels off / device batches off
    _check(m, g, qs, "td_fused=0")
    _check(m, g, qs, "batch=1")
    _check(m, g, qs, "lazy=0")


def _caterpillar(n_spine, legs):
    """A path of n_spine vertices, vertex i of it with legs[i % len(legs)] leaves."""
    edges = [(i, i + 1) for i in range(n_spine - 1)]
    v = n_spine
    for i in range(n_spine):
        for _ in range(legs[i % len(legs)]):
            edges.append((i, v))
            v += 1
    return v, edges


@pytest.mark.parametrize("K", KS)
def test_caterpillar_and_star(msbfs_pkg, K):
    """2^12 vertices: spine vertices with 0 .. 200 leaves (all weight classes and the heavy
    parents' path), and a star whose centre's whole row is leaves."""
    m = msbfs_pkg
    n, edges = _caterpillar(40, [0, 1, 2, 3, 17, 200, 16, 40, 5, 130])
    assert n <= 4096
    star0 = n
    edges += [(star0, star0 + 1 + i) for i in range(4096 - n - 1)]
    g = _graph(m, 4096, edges)
    first = [[0], [star0], [star0 + 1], [n - 1, star0 + 5], [39, 0], [star0 + 2, star0 + 3, star0]]
    qs = _query(m, 4096, first[:K], K)
    r = _check(m, g, qs)
    assert r.stats["leaf_folded"] == int((np.diff(g.rowptr) == 1).sum())
    _check(m, g, qs, "td_fused=0,dirs=TBBTB")


@pytest.fixture(scope="module")
def rmat14(msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.rmat(14, 16, 1)
    dg = _device(m, g)
    refs = {}
    yield m, g, dg, refs
    dg.close()


@pytest.fixture(scope="module")
def rmat16(msbfs_pkg):
    m = msbfs_pkg
    g = m.Graph.rmat(16, 16, 1)
    dg = _device(m, g)
    refs = {}
    yield m, g, dg, refs
    dg.close()


def _ref(m, g, refs, K):
    if K not in refs:
        qs = m.QuerySet.random(g.n, K, 16, 7)
        refs[K] = (qs, m.cpu_bfs(g, qs))
    return refs[K]


VARIANTS = [
    "",
    "bu_max=0",
    "bu_max=1000000000,lean_min=64",
    "dskip=0",
    "dskip=1,dskip3=1,lean_min=64",
    "lean=0",
    "lean=1,lean_min=64,bu_max=0",
    "push_after=0",
    "tiles=0",
    "tiles=1,tiles_w=4",
    "dirs=TBTB",          # a push level after a pull level
    "dirs=TBBTB,lean_min=64",
    "dirs=TTBB",
    "lazy=0",
    "pfx=0",
]


@pytest.mark.parametrize("K", [64, 128, 1024])
@pytest.mark.parametrize("tuning", VARIANTS)
def test_rmat14_variants(rmat14, K, tuning):
    m, g, dg, refs = rmat14
    qs, ref = _ref(m, g, refs, K)
    r = _check(m, g, qs, tuning, dg=dg, ref=ref)
    assert r.stats["leaf_folded"] == int((np.diff(g.rowptr) == 1).sum())
    assert len(r.stats) and r.stats["levels"] > 0


@pytest.mark.parametrize("K", [64, 128, 1024])
@pytest.mark.parametrize("tuning", ["", "bu_max=0,lean_min=64", "dirs=TBTB", "tiles=0,dskip=0"])
def test_rmat16_variants(rmat16, K, tuning):
    m, g, dg, refs = rmat16
    qs, ref = _ref(m, g, refs, K)
    _check(m, g, qs, tuning, dg=dg, ref=ref)


def test_trace_counts_traversed_levels(rmat14):
    m, g, dg, refs = rmat14
    qs, ref = _ref(m, g, refs, 1024)
    with m.Solver(dg, "bitpar", max_groups=qs.K, tuning="leaf=1") as s:
        r = s.run(qs)
        tr = s.level_trace()
    assert np.array_equal(r.F, ref.F)
    assert len(tr) == r.stats["levels"]


def test_consecutive_batches_and_runs(rmat14):
    """Stale leaf rows: several batches in one run (max_words=1: 64 groups each, other leaf
    sources every time) and runs with other query sets on one solver."""
    m, g, dg, refs = rmat14
    leaves = np.flatnonzero(np.diff(g.rowptr) == 1)
    with m.Solver(dg, "bitpar", max_groups=1024, tuning="leaf=1") as s, \
            m.Solver(dg, "bitpar", max_groups=1024, max_words=1, tuning="leaf=1") as s1:
        for seed in (1, 2, 3):
            rng = np.random.default_rng(seed)
            groups = [list(rng.choice(leaves, 3)) + [int(rng.integers(g.n))] for _ in range(200)]
            qs = m.QuerySet.from_groups(groups)
            ref = m.cpu_bfs(g, qs)
            for sv in (s, s1):
                r = sv.run(qs)
                assert np.array_equal(r.F, ref.F), seed
                assert r.stats["leaf_folded"] == len(leaves)
        # other word counts on the same buffers in between
        for K in (64, 128, 1024, 64):
            qs, ref = _ref(m, g, refs, K)
            assert np.array_equal(s.run(qs).F, ref.F), K


def test_folded_after_unfolded_outputs(rmat14):
    """count_edges, distances() and parents() run unfolded and write leaf rows; the folded run
    right after each must not see them."""
    m, g, dg, refs = rmat14
    qs, ref = _ref(m, g, refs, 128)
    refe = m.cpu_bfs(g, qs, count_edges=True)
    with m.Solver(dg, "bitpar", max_groups=qs.K, tuning="leaf=1") as s:
        assert np.array_equal(s.run(qs).F, ref.F)
        r = s.run(qs, count_edges=True)
        assert r.stats["leaf_folded"] == 0
        assert np.array_equal(r.F, ref.F) and np.array_equal(r.edges, refe.edges)
        assert np.array_equal(s.run(qs).F, ref.F)
        r = s.distances(qs)
        assert r.stats["leaf_folded"] == 0
        assert np.array_equal(r.F, ref.F)
        assert np.array_equal(np.where(r.dist >= 0, r.dist, 0).sum(axis=1), ref.F)
        r = s.run(qs)
        assert r.stats["leaf_folded"] > 0 and np.array_equal(r.F, ref.F)
        r = s.parents(qs)
        assert r.stats["leaf_folded"] == 0 and np.array_equal(r.F, ref.F)
        assert np.array_equal(s.run(qs).F, ref.F)


def test_off_where_not_legal_or_not_worth_it(msbfs_pkg):
    m = msbfs_pkg
    for name, g, relabel in [("rmat, user ids", m.Graph.rmat(12, 16, 1), False),
                             ("grid", m.Graph.grid(40, 60), True),
                             ("uniform", m.Graph.uniform(3000, 24000, 11), True)]:
        qs = m.QuerySet.random(g.n, 70, 3, 5)
        ref = m.cpu_bfs(g, qs)
        dg = g.to_device(0)
        if relabel:
            dg = dg.relabel_by_degree()
        try:
            for t in ("leaf=1", ""):
                with m.Solver(dg, "bitpar", max_groups=qs.K, tuning=t) as s:
                    r = s.run(qs)
                assert np.array_equal(r.F, ref.F), (name, t)
                if name != "uniform" or t == "":
                    # (leaf=1 folds the uniform graph's few leaves; auto leaves all three alone)
                    assert r.stats["leaf_folded"] == 0, (name, t)
        finally:
            dg.close()


def test_auto_folds_rmat(rmat14):
    m, g, dg, refs = rmat14
    qs, ref = _ref(m, g, refs, 1024)
    with m.Solver(dg, "bitpar", max_groups=qs.K) as s:
        s.prepare(qs)
        r = s.run(qs)
    assert np.array_equal(r.F, ref.F)
    assert r.stats["leaf_folded"] == int((np.diff(g.rowptr) == 1).sum())
    assert r.stats["builds"] == 0


@pytest.fixture(scope="module")
def rmat23(msbfs_pkg):
    m = msbfs_pkg
    dg = m.DeviceGraph.rmat(23, 16, 3, device=0)
    dg.relabel_by_degree()
    refs = {}
    yield m, dg, refs
    dg.close()


@pytest.mark.parametrize("K", [1024, 300, 128])
@pytest.mark.parametrize("tuning", ["", "push_after=0", "tiles=0", "dskip=0", "lean=0",
                                    "bu_max=0", "bu_max=1000000000", "dirs=TBT", "dirs=TBTB"])
def test_rmat23_prefix_levels(rmat23, K, tuning):
    """The graphs of more than 2^22 vertices run the first pull level prefix-wise (over the static
    tiles from 8 words on, per vertex below), the lean pass and the device-driven pull batches:
    a parent first reached by the tail push, a hub chunk, the lean pass or inside a batch. Too
    large for the CPU oracle in a test: folded against unfolded on all groups, and against the
    per-group distance solver on a sample."""
    m, dg, refs = rmat23
    if K not in refs:
        qs = m.QuerySet.random(dg.n, K, 16, seed=K)
        sub = np.arange(0, K, 89)
        with m.Solver(dg, "dist") as ds:
            refs[K] = (qs, sub, ds.run(qs.subset(sub)).F)
    qs, sub, fsub = refs[K]
    out = {}
    for leaf in (1, 0):
        t = f"leaf={leaf}" + ("," + tuning if tuning else "")
        with m.Solver(dg, "bitpar", max_groups=qs.K, tuning=t) as s:
            s.prepare(qs)
            r = s.run(qs)
            assert np.array_equal(s.run(qs).F, r.F), t  # (the leaf rows were left clean)
        assert (r.stats["leaf_folded"] > 0) == (leaf == 1), t
        out[leaf] = r.F
    assert np.array_equal(out[1], out[0]), (tuning, np.flatnonzero(out[1] != out[0])[:8])
    assert np.array_equal(out[1][sub], fsub), tuning
