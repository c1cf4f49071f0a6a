"""The level kernels' mid-loop paths: register counters that spill to LDS after 2^D - 1 tiles, LDS
queues that flush when full and are pushed into again, slab-row sums over few rows, and a last,
partial tile that is not the first. One block reaches them only after many tiles, which the
default grids give it on graphs of tens of millions of vertices; the tuning key max_grid (1 or 3
blocks here) gives it hundreds of tiles on graphs of 60000 to 260000.

Every run: F, edge counts, distances and parents equal the CPU oracle for every group, twice on
one solver (integers, no tolerance); the per-level records equal those of the same run without
the cap (the cap changes no decision and no count); and the records show that the targeted
kernels ran block_loops.TILES_MIN tiles per lane. test_block_loops_cpu.py shows on the inputs
alone that the graphs are large enough for that.

Pull kinds 'p', 't' and 'h' are taken from the graph's vertex count, isolated ids included
(pull_plan.hpp), so test_capped_grid_prefix runs them on uniform graphs padded with isolated ids
to 2^22 + 1 vertices (the big LDS hub bitmap, NarrowHubBig) and to 2^21 (the small one, NarrowHub:
the hub_small cases). The key caps k_pfx_tiles' grid (one block per CU otherwise) as well, but on
these graphs a tile never gains a bit in every pass; its counter spills are the business of
test_prefix_level_gpu.py::test_sun.

What the records cannot show is said where it applies: whether k_td_fused walked the bitmap is
inferred from the kernel's own condition (a level inside a batch, frontier >= td_bm), and the
records do not say which of k_leaf_weigh / k_leaf_weigh_list counted a level's leaves."""
import numpy as np
import pytest

import block_loops as bl

pytestmark = pytest.mark.gpu

FIELDS = ("level", "dir", "kind", "nf", "ef", "nf_next", "active")
BIG = 1 << 30

# A target (dir, kind, extent): the records must hold a level of that direction and pull kind
# whose kernels looped over TILES_MIN * max_grid * TILE entries, counted by `extent`:
#   "nf"      the frontier entering a push level (k_td_expand_small, k_td_fused, k_fix_done_rows)
#   "active"  a push level's touched list (k_td_finalize, k_count_frontier)
#   "list"    the active list entering a pull level: what the pull level before it left, or, for
#             the first one, at least what it left itself (lists only shrink)
PUSH = [("T", "", "nf"), ("T", "", "active")]
# (name, graph family, solver options, tuning, count_edges, targets)
CASES = [
    # host-driven push levels: k_td_expand_small + k_td_finalize with fused counts
    ("push", "U", {}, "dirs=TTTTTT", False, PUSH),
    # ... the edge-counting pass: k_td_finalize<false> + k_count_frontier over Lds<W, true>
    ("push_edges", "U", {}, "dirs=TTTTTT", True, PUSH),
    # first pull filtered (n), then k_bu_full (f), levels 4-5 as a device-driven batch (BuGate)
    ("pull", "U", {}, f"bu_max={BIG}", False, [("B", "n", "list"), ("B", "f", "list")]),
    ("pull_host", "U", {}, "dirs=TBBBBB", False, [("B", "n", "list"), ("B", "f", "list")]),
    # k_bu_first and its overflow pull, rows of finished vertices skipped (dskip) or written
    ("pull_lean", "U", {}, "dirs=TBBBBB,lean_min=0", False, [("B", "l", "list")]),
    ("pull_lean_rows", "U", {}, "dirs=TBBBBB,lean_min=0,dskip=0", False, [("B", "l", "list")]),
    ("pull_rows", "U", {}, "dirs=TBBBBB,dskip=0,dskip3=0", False, [("B", "f", "list")]),
    # k_bu_narrow on every level, host-driven and batched
    ("pull_narrow", "U", {}, "dirs=TBBBBB,full=0", False, [("B", "n", "list")]),
    ("pull_narrow_batch", "U", {}, f"full=0,bu_max={BIG}", False, [("B", "n", "list")]),
    # the edge-counting pass: unfused pulls + k_count_frontier<W, true, DIFF>
    ("pull_edges", "U", {}, "dirs=TBBBBB", True, [("B", "n", "list")]),
    # a push level after a row-skipping pull level: k_fix_done_rows over its frontier
    ("push_after_pull", "U", {}, "dirs=TBBTT", False, [("B", "f", "list"), ("T", "", "nf")]),
    # device-driven push batches: k_td_fused walking the bitmap / the list, the reductions of
    # several levels at once (k_level_reduce_multi); expand + finalize per level without it
    ("batch_fused_bitmap", "S", {"force_dir": 1}, "td_bm=1024", False, [("T", "", "nf")]),
    ("batch_fused_list", "S", {"force_dir": 1}, f"td_bm={BIG}", False, [("T", "", "nf")]),
    ("batch_unfused", "S", {"force_dir": 1}, "td_fused=0", False, PUSH),
    ("batch_edges", "S", {"force_dir": 1}, "", True, PUSH),
    # degree-relabelled RMAT: the load-balanced k_td_expand
    ("rmat_push", "R", {}, "dirs=TTTTTT,leaf=0", False, [("T", "", "active")]),
    # wide lists from degree 4: chunk pulls (degree scan, then two passes) + k_bu_wide_finalize
    # (their reach is the wide list's, asserted on the degrees in test_block_loops_cpu.py; the
    # records show the narrow list of the levels after the first, split at degree 1024)
    ("rmat_wide", "R", {"wide_degree": 4}, "dirs=TBBBB,leaf=0", False, [("B", "f", "list")]),
    ("rmat_wide_edges", "R", {"wide_degree": 4}, "dirs=TBBBB", True, [("B", "n", "list")]),
    # leaf folding: the lists end at the first leaf, k_leaf_weigh / k_leaf_weigh_list count them
    ("rmat_leaf", "R", {}, "leaf=1", False, [("B", "n", "list"), ("B", "f", "list")]),
    ("rmat_leaf_push", "R", {}, "leaf=1,dirs=TTTTTT", False, [("T", "", "nf")]),
    # every parent of weight 1: k_leaf_weigh's counter spills (test_block_loops_cpu.py)
    ("leafy", "L", {}, "leaf=1", False, []),
    ("leafy_push", "L", {}, "leaf=1,dirs=TTTTTTT", False, []),
    # The tree: whole runs of tiles in which one group's bit is set every time, so that a
    # counter is full when it spills (block_loops.TREE). Exact answers only: which pull kind
    # runs its levels is the planner's choice.
    ("tree_push", "T", {}, "dirs=TTTTTTTT", False, []),
    ("tree_push_edges", "T", {}, "dirs=TTTTTTTT", True, []),
    ("tree_fused_list", "T", {"force_dir": 1}, f"td_bm={BIG}", False, []),
    ("tree_fused_bitmap", "T", {"force_dir": 1}, "td_bm=1024", False, []),
    ("tree_unfused", "T", {"force_dir": 1}, "td_fused=0", False, []),
    ("tree_pull", "T", {}, "dirs=TBBBBBBB", False, []),
    ("tree_pull_lean", "T", {}, "dirs=TBBBBBBB,lean_min=0", False, []),
    ("tree_pull_narrow", "T", {}, "dirs=TBBBBBBB,full=0", False, []),
    ("tree_pull_edges", "T", {}, "dirs=TBBBBBBB", True, []),
    ("tree_pull_batch", "T", {}, f"dirs=TB,bu_max={BIG}", False, []),
]


class Inputs:
    """graphs (host + device), query sets and CPU results, each made once and left unchanged"""

    def __init__(self, m):
        self.m = m
        self.graphs, self.refs, self.base = {}, {}, {}

    def graph(self, fam, W, mg):
        name = {"U": bl.uniform_for, "S": bl.sparse_for,
                "R": lambda w, g: "R%d" % bl.rmat_scale_for(w, g),
                "L": lambda w, g: "leafy", "T": bl.tree_for}[fam](W, mg)
        if name not in self.graphs:
            g = bl.leafy_graph(self.m) if name == "leafy" else \
                bl.tree_graph(self.m, name) if fam == "T" else bl.make_graph(self.m, name)
            dg = g.to_device(0)
            if fam in "RL":
                dg.relabel_by_degree()
            self.graphs[name] = (g, dg)
        return (name,) + self.graphs[name]

    def ref(self, name, K):
        """(queries, F, edges) of the CPU oracle on the host graph (user ids)"""
        if (name, K) not in self.refs:
            g = self.graphs[name][0]
            qs = bl.tree_queries(self.m, name, K) if name in bl.TREE else \
                bl.queries(self.m, bl.LEAFY[0] if name == "leafy" else g.n, K)
            r = self.m.cpu_bfs(g, qs, count_edges=True)
            r.F.setflags(write=False)
            r.edges.setflags(write=False)
            self.refs[(name, K)] = (qs, r.F, r.edges)
        return self.refs[(name, K)]

    def close(self):
        for _, dg in self.graphs.values():
            dg.close()


@pytest.fixture(scope="module")
def inputs(msbfs_pkg):
    x = Inputs(msbfs_pkg)
    yield x
    x.close()


def _records(tr):
    return [tuple(r[f] for f in FIELDS) for r in tr]


def _run_twice(s, qs, F, E, count, what, stats=None):
    for rep in range(2):
        r = s.run(qs, count_edges=count)
        bad = np.flatnonzero(r.F != F)
        assert len(bad) == 0, (what, rep, bad[:8], r.F[bad[:8]], F[bad[:8]])
        if count:
            bad = np.flatnonzero(r.edges != E)
            assert len(bad) == 0, (what, rep, bad[:8], r.edges[bad[:8]], E[bad[:8]])
        if stats is not None:
            stats.append(r.stats)
    return s.level_trace()


def _tiles(tr, W, mg, tile=None, wide_first=0, wide_later=0):
    """per record: tiles per lane of its kernels' loops, by extent (see the targets above). A
    pull level's narrow list is the recorded list less its wide vertices, at most wide_first of
    them on the first pull level and wide_later (degree >= 1024) after it. tile: the kernel's
    own vertices per block iteration where it is not Lay<W>::TILE."""
    per = mg * (tile or bl.TILE[W])
    out = []
    for i, r in enumerate(tr):
        if r["dir"] == "T":
            ext = {"nf": r["nf"], "active": r["active"]}
        else:
            p = tr[i - 1] if i else None
            chained = p is not None and p["dir"] == "B" and p["batch"] == r["batch"] and \
                p["level"] == r["level"] - 1
            ext = {"list": max(0, p["active"] - wide_later if chained
                               else r["active"] - wide_first)}
        out.append({k: -(-v // per) for k, v in ext.items()})
    return out


def _assert_reach(tr, W, mg, targets, what, tile=None, **wide):
    tiles = _tiles(tr, W, mg, tile, **wide)
    for d, kind, ext in targets:
        hit = [t[ext] for r, t in zip(tr, tiles)
               if r["dir"] == d and r["kind"] == kind and t[ext] >= bl.TILES_MIN
               # ... and enough vertices gain a bit or stay active for the queues to fill
               and max(r["nf_next"], r["active"]) >= bl.TILES_MIN * (tile or bl.TILE[W])]
        assert hit, (what, (d, kind, ext), [(r["level"], r["dir"], r["kind"], t)
                                            for r, t in zip(tr, tiles)])


def _device_batches(tr):
    """Runs of consecutive records with one and the same ms: the levels of a device-driven batch
    (td_batch / bu_batch split the batch's wall time evenly over its levels; a host-driven level
    carries its own clock reading)."""
    runs, cur = [], [0]
    for i in range(1, len(tr)):
        if tr[i]["ms"] == tr[i - 1]["ms"] and tr[i]["dir"] == tr[i - 1]["dir"]:
            cur.append(i)
        else:
            runs.append(cur)
            cur = [i]
    runs.append(cur)
    return [r for r in runs if len(r) > 1]


def _assert_paths(name, tuning, tr, stats, g, what):
    """the paths a case is named after, where the records or the run's stats show them"""
    deg = np.diff(g.rowptr)
    if "leaf=1" in tuning:  # folded: every degree-1 vertex stayed out of the traversal
        assert all(st["leaf_folded"] == int((deg == 1).sum()) > 0 for st in stats), (what, stats)
    elif "leaf=0" in tuning:
        assert all(st["leaf_folded"] == 0 for st in stats), (what, stats)
    batches = _device_batches(tr)
    if name in ("pull", "pull_narrow_batch", "tree_pull_batch"):
        # late pull levels (from the third on) in one device-driven batch (bu_batch, BuGate)
        assert any(tr[b[0]]["dir"] == "B" for b in batches), (what, tr)
    if "dirs=" in tuning:  # forced directions: host-driven levels as far as they are forced
        forced = len(tuning.split("dirs=")[1].split(",")[0])
        assert all(tr[b[0]]["level"] > forced for b in batches), (what, batches)
    if name.startswith("batch_") or name in ("tree_fused_list", "tree_fused_bitmap",
                                             "tree_unfused"):
        # push levels in device-driven batches (td_batch): most records share their batch's ms
        assert batches and 2 * sum(len(b) for b in batches) >= len(tr), (what, tr)
    if name == "batch_fused_bitmap":
        # k_td_fused walks the bitmap on a level that is not its batch's first (the level before
        # it wrote the bitmap) and whose frontier holds td_bm = 1024 vertices: its own condition
        assert any(tr[i]["nf"] >= 1024 for b in batches for i in b[1:]), (what, tr)


@pytest.mark.parametrize("mg", bl.MAX_GRIDS)
@pytest.mark.parametrize("W", bl.WORDS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_capped_grid(inputs, case, W, mg):
    name, fam, opts, tuning, count, targets = case
    m = inputs.m
    gname, g, dg = inputs.graph(fam, W, mg)
    qs, F, E = inputs.ref(gname, bl.GROUPS[W])
    what = (name, gname, W, mg)
    key = (name, gname, W)
    if key not in inputs.base:  # the same run with every grid as computed
        with m.Solver(dg, "bitpar", max_groups=qs.K, tuning=tuning, **opts) as s:
            inputs.base[key] = _records(_run_twice(s, qs, F, E, count, what + ("uncapped",)))
    stats = []
    with m.Solver(dg, "bitpar", max_groups=qs.K, tuning=f"max_grid={mg},{tuning}", **opts) as s:
        tr = _run_twice(s, qs, F, E, count, what, stats)
    assert _records(tr) == inputs.base[key], what
    deg = np.diff(g.rowptr)
    wide = dict(wide_first=int((deg >= opts.get("wide_degree", bl.WIDE_DEFAULT)).sum()),
                wide_later=int((deg >= 1024).sum()))
    print(what, [(r["level"], r["dir"] + r["kind"], t)
                 for r, t in zip(tr, _tiles(tr, W, mg, **wide))])
    _assert_reach(tr, W, mg, targets, what, **wide)
    _assert_paths(name, tuning, tr, stats, g, what)


# The prefix level ('p': per-vertex prefix pull + k_push_tail; 't': the tiles, here for the capped
# k_push_tail_after / k_push_tail and big-vertex finalize around them) and the LDS-hub pull ('h').
# HALF = half the graph's vertices as the prefix bound: the other half's frontier vertices push
# (k_push_tail has work), and the lists are split by prefix length where HALF <= 131072.
# td_fused=0: on these low-degree graphs the batch is then lazy, as on every graph with hubs, and a
# lazy batch's first pull level is filtered whatever level 1 visited (with 512 groups or more it
# visits most of a 60000-vertex graph, and an unfiltered level 2 is a plain k_bu_full level). The
# edge-counting pass is never lazy: its cases stop at 4 words, where level 1 visits under half.
# (name, kind of level 2, tile table, words, tuning, count_edges)
PFX = "dirs=TBBBBB,leaf=0,td_fused=0"
PREFIX_CASES = [
    ("prefix", "p", bl.PFX_TILE, bl.WORDS, PFX + ",tiles=0", False),
    ("prefix_tail", "p", bl.PFX_TILE, bl.WORDS, PFX + ",tiles=0,pfx_h=HALF", False),
    ("prefix_edges", "p", bl.PFX_TILE, (1, 2, 4), PFX + ",tiles=0,pfx_h=HALF", True),
    ("tiled", "t", None, (8, 16), PFX + ",pfx_h=HALF", False),
    ("tiled_push_before", "t", None, (8, 16), PFX + ",push_after=0", False),
    ("hub", "h", bl.HUB_TILE, bl.WORDS, PFX + ",pfx=0", False),
    ("hub_all_levels", "h", bl.HUB_TILE, bl.WORDS, PFX + ",pfx=0,filter_frac=2", False),
    # Those two run NarrowHubBig (n > 2^22). Padded to PAD_HUB ids the same graphs take the small
    # hub bitmap, NarrowHub, and no prefix level whatever pfx says. Both variants record 'h':
    # the vertex count asserted below is what tells them apart.
    ("hub_small", "h", bl.HUB_TILE, bl.WORDS, PFX, False),
    ("hub_small_all_levels", "h", bl.HUB_TILE, bl.WORDS, PFX + ",filter_frac=2", False),
]


@pytest.mark.parametrize("mg", bl.MAX_GRIDS)
@pytest.mark.parametrize("case,W", [(c, W) for c in PREFIX_CASES for W in c[3]],
                         ids=[f"{c[0]}-{W}" for c in PREFIX_CASES for W in c[3]])
def test_capped_grid_prefix(inputs, case, W, mg):
    name, kind, tiles, _, tuning, count = case
    m = inputs.m
    tile = (tiles or bl.PFX_TILE)[W]
    pad_n = bl.PAD_HUB if name.startswith("hub_small") else bl.PAD_N
    gname = bl.padded_for(tile, mg) + ("" if pad_n == bl.PAD_N else "_hub")
    if gname not in inputs.graphs:
        core, padded = bl.padded_graph(m, gname.split("_")[0], pad_n)
        inputs.graphs[gname] = (core, padded.to_device(0).relabel_by_degree())
    core, dg = inputs.graphs[gname]
    assert dg.n == pad_n and dg.hybrid_extent() == core.n
    # (pull_plan.hpp: hub_lds from kHubW * 32 * 4 vertices on, hub_big_graph above kHubBig * 32 * 4)
    assert dg.n > 14336 * 128 and (dg.n <= 32768 * 128) == name.startswith("hub_small")
    # the oracle runs on the unpadded graph: the same CSR without the isolated ids, which no
    # group can reach (its distance array is per group, 2^22 entries each on the padded one)
    qs, F, E = inputs.ref(gname, bl.GROUPS[W])
    tuning = tuning.replace("HALF", str(core.n // 2))
    what = (name, gname, W, mg)
    key = (name, gname, W)
    if key not in inputs.base:
        with m.Solver(dg, "bitpar", max_groups=qs.K, tuning=tuning) as s:
            inputs.base[key] = _records(_run_twice(s, qs, F, E, count, what + ("uncapped",)))
    stats = []
    with m.Solver(dg, "bitpar", max_groups=qs.K, tuning=f"max_grid={mg},{tuning}") as s:
        tr = _run_twice(s, qs, F, E, count, what, stats)
    assert _records(tr) == inputs.base[key], what
    assert (tr[1]["level"], tr[1]["dir"], tr[1]["kind"]) == (2, "B", kind), (what, tr[1])
    if name.endswith("all_levels"):
        assert all(r["kind"] == "h" for r in tr if r["dir"] == "B"), (what, tr)
    _assert_paths(name, tuning, tr, stats, core, what)
    if tiles is None:
        return  # (k_pfx_tiles: the records hold no list it loops over; see test_prefix_level_gpu.py)
    deg = np.diff(core.rowptr)
    wide = dict(wide_first=int((deg >= bl.WIDE_DEFAULT).sum()), wide_later=int((deg >= 1024).sum()))
    print(what, [(r["level"], r["dir"] + r["kind"], t)
                 for r, t in zip(tr, _tiles(tr, W, mg, tile, **wide))])
    _assert_reach(tr, W, mg, [("B", kind, "list")], what, tile, **wide)


@pytest.mark.parametrize("K", [bl.GROUPS[1], 520])  # one word; 16 words (the fewest groups)
@pytest.mark.parametrize("out", ["distances", "parents"])
def test_capped_grid_records(inputs, out, K):
    """distances() and parents() with one block: the record kernels' loops over the new frontier
    (k_record_levels, k_record_mark, k_record_parents, k_record_commit) behind the edge-counting
    levels. The graph keeps its ids, so the device rows are the host graph's."""
    m = inputs.m
    gname, g, dg = inputs.graph("U", 1, 1)
    qs = bl.queries(m, g.n, K)
    ref = m.cpu_bfs(g, qs, parents=(out == "parents"), distances=True)
    with m.Solver(dg, "bitpar", max_groups=K, tuning="max_grid=1") as s:
        r = s.parents(qs) if out == "parents" else s.distances(qs)
        tr = s.level_trace()
    assert np.array_equal(r.F, ref.F)
    assert np.array_equal(r.dist, ref.dist)
    if out == "parents":
        assert np.array_equal(r.parent, ref.parent)
    # the new frontier of some level is TILES_MIN blocks of 256 threads long at the least
    assert max(t["nf_next"] for t in tr) >= bl.TILES_MIN * 256, tr


@pytest.mark.parametrize("W", [2, 16])
def test_capped_grid_hybrid(inputs, W):
    """The hybrid mode's phases, two emulated ranks on one GPU, one block: phase A pulls and packs
    every second vertex (k_pack_words), phase C rebuilds the state (k_hybrid_setup) and runs the
    remaining levels. The graph is twice need(W, 1) so that each rank's half is long enough."""
    from msbfs.parallel import hybrid as H
    m = inputs.m
    gname, g, dg = inputs.graph("U", W, 3)
    assert g.n // 2 >= bl.need(W, 1)
    qs, F, _ = inputs.ref(gname, bl.GROUPS[W])
    with m.Solver(dg, "bitpar", max_groups=qs.K, tuning="max_grid=1") as s:
        for rep in range(2):
            assert np.array_equal(H.emulate_ranks(s, qs, 2), F), (W, rep)
