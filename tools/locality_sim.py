#!/usr/bin/env python3
"""Which neighbour rows hit a cache at a pull level, under two vertex orders? (CPU model, no GPU.)

Extends tools/pull_steps_sim.py: RMAT graph, K groups of `size` random sources, exact per-group
BFS. At pull level L the active vertices (some alive group has not visited them) are taken in id
order; each ORs its neighbours' rows in row order until every such group is covered or its row
ends (a first step of c1 rows, then steps of cs rows, as the kernels gather them). The row ids
form one stream, and one LRU cache of rows sees all of it; a cache of n / 2048 rows stands for
one XCD's 4-MB L2 against 2^26 rows of 128 bytes.

The two orders:
  degree    degree descending, ties by id (the relabelling without the locality key)
  top-hub   degree descending, then the id (in the degree order) of the vertex's highest-degree
            neighbour, then id (MSBFS_RELABEL_LOCALITY=1)

    python tools/locality_sim.py --scale 18 --groups 128 --level 3
    python tools/locality_sim.py --scale 18 --groups 128 --level 3 --c1 8 --cs 8
"""
import argparse
import collections
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def orders(g):
    """old -> new maps of the two orders."""
    n = g.n
    ids = np.arange(n, dtype=np.int64)
    deg = g.degrees()
    prov = np.empty(n, np.int64)
    prov[np.lexsort((ids, -deg))] = ids
    key2 = np.full(n, np.iinfo(np.uint32).max, np.int64)
    rows = np.flatnonzero(deg > 0)
    key2[rows] = np.minimum.reduceat(prov[g.col], g.rowptr[rows])
    hub = np.empty(n, np.int64)
    hub[np.lexsort((ids, key2, -deg))] = ids
    return {"degree": prov, "top-hub": hub}


def row_stream(g, new_id, qs, args):
    """Row ids gathered at pull level args.level, in the order the active list reads them."""
    import scipy.sparse as sp

    deg = g.degrees()
    src = np.repeat(np.arange(g.n), deg)
    A = sp.csr_matrix((np.ones(len(g.col), np.int8), (new_id[src], new_id[g.col])),
                      shape=(g.n, g.n))
    A.sort_indices()
    rowptr, col = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    d = np.diff(rowptr)
    K, L = args.groups, args.level
    W = (K + 63) // 64
    vis = np.zeros((g.n, W), np.uint64)   # groups with dist <= L - 1
    unv = np.zeros((g.n, W), np.uint64)   # alive groups with dist >= L
    for j in range(K):
        srcs = new_id[qs.ids[qs.off[j]:qs.off[j + 1]]]
        seen = np.zeros(g.n, bool)
        seen[srcs] = True
        fr = seen.copy()
        for _ in range(L - 1):
            nxt = (A @ fr.astype(np.int8)) > 0
            fr = nxt & ~seen
            seen |= fr
        if not fr.any():
            continue
        bit = np.uint64(1) << np.uint64(j % 64)
        vis[seen, j // 64] |= bit
        unv[~seen, j // 64] |= bit
    active = np.nonzero((unv != 0).any(axis=1) & (d > 0) & (d <= args.wide))[0]
    k = np.zeros(len(active), np.int64)
    acc = np.zeros((len(active), W), np.uint64)
    need = unv[active]
    open_ = np.ones(len(active), bool)
    pos = 0
    while open_.any():
        idx = np.nonzero(open_ & (d[active] > pos))[0]
        if len(idx) == 0:
            break
        acc[idx] |= vis[col[rowptr[active[idx]] + pos]]
        k[idx] = pos + 1
        cov = ((acc[idx] & need[idx]) == need[idx]).all(axis=1)
        open_[idx[cov]] = False
        open_[np.nonzero(open_ & (d[active] <= pos + 1))[0]] = False
        pos += 1
    # rows actually gathered: whole steps, clipped to the row
    steps = np.where(k <= args.c1, 0, (k - args.c1 + args.cs - 1) // args.cs)
    got = np.minimum(args.c1 + steps * args.cs, d[active])
    start = np.repeat(rowptr[active], got)
    within = np.arange(int(got.sum())) - np.repeat(np.cumsum(got) - got, got)
    return col[start + within], len(active), float((k == 1).mean()) if len(k) else 0.0


def lru_hit_rate(stream, rows):
    cache = collections.OrderedDict()
    hits = 0
    for r in stream.tolist():
        if r in cache:
            cache.move_to_end(r)
            hits += 1
        else:
            cache[r] = None
            if len(cache) > rows:
                cache.popitem(last=False)
    return hits / max(1, len(stream))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--groups", type=int, default=128)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--c1", type=int, default=1, help="rows of the first step (k_bu_full: 8)")
    ap.add_argument("--cs", type=int, default=1, help="rows of every later step")
    ap.add_argument("--wide", type=int, default=1024, help="wider rows go to the chunk kernels")
    ap.add_argument("--cache-div", type=int, nargs="+", default=[2048],
                    help="cache sizes as n / DIV rows")
    args = ap.parse_args()

    import msbfs
    g = msbfs.Graph.rmat(args.scale, 16, 1)
    qs = msbfs.QuerySet.random(g.n, 1024, args.size, 7)
    out = {"scale": args.scale, "groups": args.groups, "level": args.level, "c1": args.c1,
           "cs": args.cs, "orders": {}}
    for name, new_id in orders(g).items():
        stream, nact, first = row_stream(g, new_id, qs, args)
        out["orders"][name] = {
            "active": nact, "rows": int(len(stream)), "first_row_covers": round(first, 4),
            "hit_rate": {f"n/{dv}": round(lru_hit_rate(stream, max(1, g.n // dv)), 4)
                         for dv in args.cache_div}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
