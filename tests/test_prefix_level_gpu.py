"""The first pull level (level 2: k_pfx_tiles or the per-vertex prefix pull, the sparse codes, the
tail push before or after it, the big vertices' partial tiles and finalize) against the CPU
oracle, for every group, exactly, on the designed inputs of prefix_graphs.py.
test_prefix_level_cpu.py shows on the inputs alone which boundaries they meet: prefix lengths
around a round (256), a partial tile (1024) and two of them, a carrier alone at the first or the
last prefix entry, level-1 vertices at internal ids H - 1 and H = 458752, rows of 1, 2, 3, 4 and
65+ groups at word seams, vertices reached by the push alone, by the pull alone and by both, tiles
without any entry, leaves around the pushers. Those facts are about the bound H = 458752: the
tiled level always runs there, the per-vertex prefix pull ('p') only where the case says
pfx_h=458752 or the source count gives it (see CASES for the bound of every 'p' case); at another
bound a 'p' case shows exactness against the oracle and no more.

Every case runs profile(bins="all") twice and run() once on one solver: F, reach, eccentricity and
the whole level histogram equal the oracle's for every group (integers: no tolerance), and the
record of level 2 shows the pull kind the case is named after. profile() runs the kernels of
run(), so its histogram's level-2 column pins the level's per-group counts, which F alone (a
weighted sum over levels) would not.

The sun graph (prefix_graphs.sun_graph) is there for k_pfx_tiles' register counters
(GroupCounts<W, 5, ...>: a spill every 31 epilogue passes): with the tuning key max_grid its grid
is 1 or 3 blocks, every wave runs block_loops.TILES_MIN tiles or more, and every vertex of every
tile gains every group, so each counter is full whenever it spills. The level records and the run
stats do not show a kernel's grid, so that the cap reached k_pfx_tiles cannot be asserted here."""
import numpy as np
import pytest

import block_loops as bl
import prefix_graphs as pg
from degree_graphs import relabel_oracle
from profile_oracle import check

pytestmark = pytest.mark.gpu

DIRS = "dirs=TBBBBBBB"


def _t(*parts):
    return ",".join(p for p in parts if p)
FIELDS = ("level", "dir", "kind", "nf", "ef", "nf_next", "active")
WORDS = {64: 1, 128: 2, 256: 4, 512: 8, 1024: 16}


class Inputs:
    """one graph (host, device, relabelling checked against the numpy oracle), its 1024 groups and
    the CPU oracle per group count, each made once and left unchanged"""

    def __init__(self, m, g, queries):
        self.m, self.g = m, g
        self.core, padded = pg.host_graphs(m, g)
        self.o2n = relabel_oracle(padded, locality=True)[0]
        self.dg = padded.to_device(0).relabel_by_degree()
        # the census (and the sun's layout) speak of these ids: the run must use them
        assert np.array_equal(self.dg.relabel_map(), self.o2n)
        assert self.dg.n == pg.PAD_N and self.dg.hybrid_extent() == g.n_core
        self.qs = queries(self)
        self.refs, self.base = {}, {}

    def ref(self, K):
        """(queries, (F, reach, ecc, hist)) of the first K groups, on the unpadded graph: the same
        CSR without the isolated ids, which no group reaches"""
        if K not in self.refs:
            qs = self.qs.subset(range(K))
            r = self.m.cpu_bfs(self.core, qs, profile=True, bins="all")
            for a in (r.F, r.reach, r.ecc, r.hist):
                a.setflags(write=False)
            self.refs[K] = (qs, (r.F, r.reach, r.ecc, r.hist))
        return self.refs[K]


@pytest.fixture(scope="module")
def design(msbfs_pkg):
    x = Inputs(msbfs_pkg, pg.boundary_graph(1),
               lambda i: pg.boundary_queries(i.m, i.g, i.o2n, 1024))
    c = pg.census(x.g, x.o2n, x.qs)
    print("census", {k: v for k, v in c.items() if not k.startswith("rows_")})
    yield x
    x.dg.close()


@pytest.fixture(scope="module")
def sun(msbfs_pkg):
    x = Inputs(msbfs_pkg, pg.sun_graph(), lambda i: pg.sun_queries(i.m, i.g, 1024))
    yield x
    x.dg.close()


def _records(tr):
    return [tuple(r[f] for f in FIELDS) for r in tr]


def _run(x, K, tuning, kind, what):
    """profile twice, run once on one solver, everything against the oracle; level 2 is a pull of
    `kind`. Returns (records of run(), its stats)."""
    qs, ora = x.ref(K)
    with x.m.Solver(x.dg, "bitpar", max_groups=K, tuning=tuning) as s:
        for rep in range(2):
            r = s.profile(qs, bins="all")
            check(r, ora, r.hist.shape[1], (what, tuning, "profile", rep))
            assert r.hist.shape[1] >= int(ora[2].max()) + 2 and not r.hist[:, -1].any()
            tp = _records(s.level_trace())
            assert tp[1][:3] == (2, "B", kind), (what, tuning, tp[1])
        r = s.run(qs)
        bad = np.flatnonzero(r.F != ora[0])
        assert len(bad) == 0, (what, tuning, "run", bad[:8], r.F[bad[:8]], ora[0][bad[:8]])
        tr = _records(s.level_trace())
        # (profile() ran the levels of run(): level, direction, kind, frontier)
        assert [t[:4] + t[5:6] for t in tr] == [t[:4] + t[5:6] for t in tp], (what, tuning)
        return tr, r.stats


def _base(x, K, tuning, kind):
    """the records of the same run with every grid as computed"""
    if (K, tuning) not in x.base:
        x.base[(K, tuning)] = _run(x, K, tuning, kind, ("uncapped", K))[0]
    return x.base[(K, tuning)]


TILED = ["", "push_after=0", "codes=0", "push_after=0,codes=0",
         # sparse codes for every id (code_bound returns 0: no vertex has 2^38 neighbours), for
         # none (every vertex has degree >= 0), and for the ids of degree < 16 or 32 only (the
         # first-entry carriers and the targets keep dense rows)
         "tiles_code_deg=1e9", "tiles_code_deg=0", "tiles_code_deg=0.05"]
FULL_H = f"pfx_h={pg.H}"
CASES = (
    # Per-vertex prefix pull, every vertex reads its pushed row (no stamps). Its bound without
    # pfx_h is BitparSolver::pfx_bound_n's: the ids of degree >= 2^k, 2^k <= n / (64 W sources),
    # at least 1024 ids. With the 292 / 489 / 746 sources of 64 / 128 / 256 groups that degree is
    # 128 / 64 / 16, which 26 vertices have at the most: H = 1024 in the default case as with
    # pfx_h=1024, and all ids from 1024 on push. FULL_H: the bound of the census.
    [(K, t, "p") for K in (64, 128, 256) for t in (FULL_H, "", "pfx_h=1024")] +
    # ... with stamps. Without pfx_h: 512 groups (1258 sources) H = the about 23000 ids of
    # degree >= 4; 1024 groups (2287 sources) H = 458752 as with FULL_H
    [(K, _t("tiles=0", t), "p") for K in (512, 1024) for t in (FULL_H, "", "codes=0",
                                                               _t("codes=0", FULL_H))] +
    # tiles
    [(256, "tiles_w=4", "t"), (256, "tiles_w=4,push_after=0", "t")] +
    [(K, t, "t") for K in (512, 1024) for t in TILED])


@pytest.mark.parametrize("K,tuning,kind", CASES, ids=[f"{c[0]}-{c[2]}-{c[1]}" for c in CASES])
def test_design(design, K, tuning, kind):
    t = _t(DIRS, "leaf=0", tuning)
    tr, st = _run(design, K, t, kind, ("design", K))
    assert st["leaf_folded"] == 0
    design.base[(K, t)] = tr


@pytest.mark.parametrize("K,tuning", [(256, "tiles_w=4"), (1024, "")])
def test_design_push_next(design, K, tuning):
    """a push level right after the tiled one: its frontier list comes from the level's frontier
    bitmap (k_bitmap_list)"""
    tr, _ = _run(design, K, _t("dirs=TBT", "leaf=0", tuning), "t", ("push_next", K))
    assert tr[2][:2] == (3, "T"), tr[2]


@pytest.mark.parametrize("tuning", TILED)
@pytest.mark.parametrize("K", [512, 1024])
def test_design_leaf_fold(design, K, tuning):
    """leaf folding: the tile table ends at the first leaf, the pushes skip the leaves (vmax)"""
    tr, st = _run(design, K, _t(DIRS, "leaf=1", tuning), "t", ("leaf", K))
    deg = np.diff(design.core.rowptr)
    assert st["leaf_folded"] == int((deg == 1).sum()) > 0, st


@pytest.mark.parametrize("mg", bl.MAX_GRIDS)
@pytest.mark.parametrize("tuning", ["", "push_after=0"])
@pytest.mark.parametrize("K", [256, 512, 1024])
def test_design_capped(design, K, tuning, mg):
    """max_grid blocks for the tiles (16 * max_grid tiles in flight), the pushes and the finalize"""
    t = _t(DIRS, "leaf=0", "tiles_w=4" if K == 256 else "", tuning)
    base = _base(design, K, t, "t")
    tr, _ = _run(design, K, f"max_grid={mg},{t}", "t", ("capped", K, mg))
    assert tr == base, (K, tuning, mg)


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("K", [512, 1024])
def test_design_hybrid(design, K, world):
    """phase A of `world` emulated ranks: tiles of strided vertices, one bitmap bit per vertex,
    k_push_tail's ownership test by mask (2, 4) and by modulo (3)"""
    import torch
    from msbfs.parallel import hybrid
    qs, ora = design.ref(K)
    with design.m.Solver(design.dg, "bitpar", max_groups=K) as s:
        for rep in range(2):
            F = hybrid.emulate_ranks(s, qs, world)
            bad = np.flatnonzero(F != ora[0])
            assert len(bad) == 0, (K, world, rep, bad[:8], F[bad[:8]], ora[0][bad[:8]])
        # emulate_ranks leaves the records of its last phase C; one more phase A of the last rank
        # (the dense exchange buffer sized as emulate_ranks sizes it) leaves its own: level 2 ran
        # over the tiles. (That the tail push ran before them, push_after being off for a vertex
        # partition, is the planner's decision, pinned in csrc/tests/host_selftest.cpp: no
        # record names the push kernel.)
        n_eff = design.dg.hybrid_extent()
        wbeg = hybrid.word_split(K, world)
        ss, _ = hybrid.split_sizes(n_eff, wbeg, world - 1)
        buf = torch.empty(max(1, sum(ss)), dtype=torch.int64, device=torch.device("cuda", 0))
        s.hybrid_phase_a(qs, world - 1, world, n_eff, False, wbeg, buf.data_ptr(), coded=False)
        torch.cuda.synchronize()
        tr = _records(s.level_trace())
        assert [t[:3] for t in tr] == [(1, "T", ""), (2, "B", "t")], tr


@pytest.mark.parametrize("mg", bl.MAX_GRIDS)
@pytest.mark.parametrize("tuning", ["", "push_after=0"])
@pytest.mark.parametrize("K", [256, 512, 1024])
def test_sun(sun, K, tuning, mg):
    nbody = sun.g.nbody
    # The body alone fills nbody // VT tiles or more (a tile holds VT vertices at the most), each
    # with an epilogue pass or more. The tile table starts with the hub's partial tiles, which run
    # none, and tile t goes to wave t % (TILE_WAVES * mg): of any run of consecutive tiles a wave
    # gets the run's length // (TILE_WAVES * mg) at the least, so of the body's TILES_MIN or more,
    # four spill periods of 2^5 - 1 passes
    per_wave = nbody // pg.VT // (pg.TILE_WAVES * mg)
    assert per_wave >= bl.TILES_MIN > 4 * 31
    t = _t(DIRS, "leaf=0", "tiles_w=4" if K == 256 else "", tuning)
    base = _base(sun, K, t, "t")
    tr, _ = _run(sun, K, f"max_grid={mg},{t}", "t", ("sun", K, mg))
    assert tr == base, (K, tuning, mg)
    # level 1 is the hub (and each handle's leaf), level 2 every body vertex and handle
    assert tr[0][3] == K and tr[1][3] == K + 1 and tr[1][5] == nbody + pg.SUN_HANDLES, tr[:2]
    # (The records do not hold the grid of k_pfx_tiles: that max_grid reached it cannot be
    # asserted here.)
