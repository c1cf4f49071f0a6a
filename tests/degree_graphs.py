"""Graphs with prescribed degrees, and numpy oracles of the graph preprocessing (numpy only).

The kernels in front of every solver branch on a row's length: the four buckets of the row sort
(2..64, 65..1024, 1025..16384, more), the short and the long locality key (256), the 1024-entry
hub chunks of the pulls, the narrow, wide and wider pulls (32, 64, 128) and the parent search
(msbfs_parents_wide_degree()). boundary_graph() puts one vertex at each such length, one below
and one above, into a graph small enough to compare whole arrays; sorted_csr() and
relabel_oracle() say what the row sort and the degree relabelling have to make of it.
"""
import numpy as np

# every boundary named above at -1, 0, +1, and two rows in the > 16384 bucket
DEFAULT_DEGREES = (2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025,
                   2047, 2048, 2049, 3073, 16383, 16384, 16385, 20001)
K2_COMPONENTS = 5
ISOLATED = 7


def boundary_graph(degrees=DEFAULT_DEGREES, seed=1):
    """(n, u, v, hubs): a multigraph in which vertex hubs[i] has degree exactly degrees[i].

    The hubs lie on a path in the order given, so a BFS from one end meets a hub on every level.
    One hub carries a self-loop (2 entries of its own row), one pair of neighbouring hubs a
    second, duplicate edge; both go to the first hubs from the 6th / 8th on (wrapping round)
    whose degree has room for them, and are left out if none has. Spokes fill every hub up to
    its degree: each third one is a 2-path (a degree-2 vertex, then a leaf), the others leaves.
    K2_COMPONENTS components of two degree-1 vertices (a leaf whose only neighbour is a leaf)
    and ISOLATED isolated vertices (one more if n would be a multiple of 64) come last. Vertex
    ids are scrambled and the edges shuffled by `seed`; u, v are int32."""
    D = [int(d) for d in degrees]
    H = len(D)
    if H == 0:
        raise ValueError("at least one hub")
    deg = np.zeros(H, dtype=np.int64)
    if H > 1:
        deg[[0, H - 1]] += 1
        deg[1:H - 1] += 2
    for i in range(H):
        if D[i] < deg[i]:
            raise ValueError(f"degree {D[i]} of hub {i} is below its {deg[i]} path edges")
    eu = list(range(H - 1))
    ev = list(range(1, H))
    for i in (np.arange(H) + 5) % H:                      # the self-loop
        if D[i] - deg[i] >= 2:
            eu.append(int(i))
            ev.append(int(i))
            deg[i] += 2
            break
    for i in (np.arange(H - 1) + 7) % max(H - 1, 1):      # the duplicate edge
        if D[i] - deg[i] >= 1 and D[i + 1] - deg[i + 1] >= 1:
            eu.append(int(i))
            ev.append(int(i) + 1)
            deg[i] += 1
            deg[i + 1] += 1
            break
    us, vs = [np.array(eu, np.int64)], [np.array(ev, np.int64)]
    nxt = H
    for i in range(H):
        need = int(D[i] - deg[i])
        long_ = (np.arange(need) % 3 == 0).astype(np.int64)    # spoke j is a 2-path
        first = nxt + np.arange(need) + np.cumsum(long_) - long_  # the spoke's first vertex
        us += [np.full(need, i, np.int64), first[long_ == 1]]
        vs += [first, first[long_ == 1] + 1]
        nxt += need + int(long_.sum())
    k2 = nxt + 2 * np.arange(K2_COMPONENTS)
    us.append(k2)
    vs.append(k2 + 1)
    nxt += 2 * K2_COMPONENTS + ISOLATED
    if nxt % 64 == 0:
        nxt += 1
    n = nxt
    u, v = np.concatenate(us), np.concatenate(vs)
    rng = np.random.default_rng(seed)
    p = rng.permutation(n)
    order = rng.permutation(len(u))
    return (n, p[u][order].astype(np.int32), p[v][order].astype(np.int32),
            p[:H].astype(np.int32))


def sorted_csr(n, u, v):
    """(rowptr int64[n + 1], col int32[2m]) of the symmetric CSR with every row ascending; a
    self-loop puts its vertex into its own row twice, a duplicate edge stays."""
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    src, dst = np.concatenate([u, v]), np.concatenate([v, u])
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=rowptr[1:])
    return rowptr, dst[np.lexsort((dst, src))].astype(np.int32)


def rows_ascending(rowptr, col):
    """col with every row of the CSR sorted (numpy; to compare rows as multisets)"""
    col = np.asarray(col)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return col[np.lexsort((col, rows))]


def _oracle_map(host, locality=True):
    """old2new for (degree descending, key2 ascending, old id ascending), key2[v] = the smallest
    id, in the degree-only order, among v's neighbours (UINT32_MAX for an isolated vertex).
    locality=False: the degree-only order itself."""
    n = host.n
    ids = np.arange(n, dtype=np.int64)
    deg = np.diff(host.rowptr)
    prov = np.empty(n, np.int64)
    prov[np.lexsort((ids, -deg))] = ids
    if not locality:
        return prov, deg
    key2 = np.full(n, np.iinfo(np.uint32).max, np.int64)
    rows = np.flatnonzero(deg > 0)
    key2[rows] = np.minimum.reduceat(prov[host.col], host.rowptr[rows])
    o2n = np.empty(n, np.int64)
    o2n[np.lexsort((ids, key2, -deg))] = ids
    return o2n, deg


def relabel_oracle(host, locality):
    """(old2new, rowptr, col) of the degree relabelling of a host CSR (n, rowptr, col): new row i
    is sort(old2new[old row of new2old[i]])."""
    o2n, deg = _oracle_map(host, locality)
    new2old = np.empty(host.n, np.int64)
    new2old[o2n] = np.arange(host.n)
    rowptr = np.zeros(host.n + 1, dtype=np.int64)
    np.cumsum(deg[new2old], out=rowptr[1:])
    rows = o2n[np.repeat(np.arange(host.n), deg)]
    vals = o2n[host.col]
    return o2n.astype(np.int32), rowptr, vals[np.lexsort((vals, rows))].astype(np.int32)
