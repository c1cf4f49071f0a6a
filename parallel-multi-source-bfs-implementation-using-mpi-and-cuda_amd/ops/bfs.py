"""Multi-source BFS operators: F(U_k) for every query group.

F(U) = sum over vertices v reachable from U of dist(U, v) (reference GPUMultiSourceBFS +
ComputeFofU, main.cu:40-89). Sources outside [0, n) are ignored (main.cu:49); unreachable
vertices contribute nothing (main.cu:84-85).

Algorithms (all give identical F — it is an exact integer sum):
  bitpar  — 64*W groups per pass, direction-optimising, per-group sums on chip (default, K > 1)
  dist    — per-group distance array, direction-optimising (default for K == 1)
  topdown — per-group, top-down only (queue + load-balanced edge expansion)
  sweep   — the reference algorithm (thread per vertex, full sweep per level), on-device sum
  cpu     — host threads (query-parallel), the "serial CPU BFS" config and oracle
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Union

import numpy as np

from . import native
from ..models.graph import DeviceGraph, Graph
from ..models.queries import QuerySet


@dataclass
class BfsResult:
    F: np.ndarray                      # int64[K]
    edges: Optional[np.ndarray] = None  # int64[K], Graph500 traversed edges per group (if asked)
    stats: dict = field(default_factory=dict)
    # int32[K, n] per-vertex distances (original vertex ids; -1 unreached) of a distances() /
    # distances=True call; None otherwise, and when they went to a device buffer (out_ptr)
    dist: Optional[np.ndarray] = None
    # int32[K, n] BFS parents (original vertex ids; a source is its own parent, -1 unreached) of
    # a parents() / parents=True call; None otherwise, and when they went to device buffers
    parent: Optional[np.ndarray] = None
    # the level profile of a profile() / profile=True call (None otherwise): reach int64[K]
    # (vertices reached, sources included), ecc int32[K] (largest distance, -1 for a group
    # without a valid source), hist int64[K, bins] (vertices per distance; the last column is
    # the tail: every vertex at distance >= bins - 1)
    reach: Optional[np.ndarray] = None
    ecc: Optional[np.ndarray] = None
    hist: Optional[np.ndarray] = None


def _host_dist_out(K: int, n: int, out: Optional[np.ndarray], ld: Optional[int]):
    """The host matrix a distance call writes and its row stride: `out` (C-contiguous int32
    [K, >= n], written in place, columns >= n untouched) or a fresh [K, ld or n] array."""
    if out is None:
        ld = n if ld is None else int(ld)
        if ld < n:
            raise ValueError("ld must be at least n")
        return np.full((K, ld), -1, dtype=np.int32), ld
    if (out.dtype != np.int32 or out.ndim != 2 or not out.flags.c_contiguous
            or out.shape[0] != K or out.shape[1] < n):
        raise ValueError("out must be a C-contiguous int32 array of shape [K, >= n]")
    if ld is not None and int(ld) != out.shape[1]:
        raise ValueError("ld must equal out.shape[1]")
    return out, out.shape[1]


def _profile_call(K: int, bins, call) -> tuple:
    """Run call(F, reach, ecc, hist, nbins) for `bins` columns; bins="all": 64 columns, and once
    more with max(ecc) + 2 if a group reaches the tail (so that every level has its own column
    and the tail column stays zero). Returns (F, reach, ecc, hist)."""
    every = isinstance(bins, str)
    if every and bins != "all":
        raise ValueError('bins must be a positive integer or "all"')
    nbins = 64 if every else int(bins)
    if nbins < 1:
        raise ValueError("bins must be at least 1")
    while True:
        F = np.zeros(K, dtype=np.int64)
        reach = np.zeros(K, dtype=np.int64)
        ecc = np.full(K, -1, dtype=np.int32)
        hist = np.zeros((K, nbins), dtype=np.int64)
        if K:
            call(F, reach, ecc, hist, nbins)
        if every and K and int(ecc.max()) >= nbins - 1:
            nbins = int(ecc.max()) + 2
            continue
        return F, reach, ecc, hist


class Solver:
    """Reusable device workspace for one graph + algorithm (allocated once, like the reference's
    one-time cudaMalloc of the distance array main.cu:294-295, but for all algorithms)."""

    def __init__(self, graph: DeviceGraph, algo: str = "auto", max_groups: int = 1024,
                 alpha: float = 0.0, beta: float = 0.0, wide_degree: int = 0,
                 force_dir: int = 0, max_words: int = 0, tuning=None):
        """tuning: algorithm tuning keys of the bit-parallel solver, a dict {"gamma2": 0.5, ...}
        or a "key=value,..." string (see msbfs_solver_tune in csrc/include/msbfs/msbfs.h);
        unknown keys raise MsbfsError."""
        if algo not in native.ALGOS or algo == "cpu":
            raise ValueError(f"unknown device algorithm {algo!r}")
        self.graph = graph
        self.algo = algo
        h = C.c_void_p()
        native.check(native.lib().msbfs_solver_create(graph.handle, native.ALGOS[algo],
                                                      max(1, int(max_groups)), C.byref(h)))
        self._h = h
        if alpha or beta or wide_degree or force_dir or max_words:
            o = native.Options(alpha, beta, wide_degree, force_dir, max_words)
            native.check(native.lib().msbfs_solver_set_options(self._h, C.byref(o)))
        if tuning:
            self.tune(tuning)

    def prepare(self, queries: Optional[QuerySet] = None, stream: Optional[int] = None) -> None:
        """Build the graph-derived tables and worst-case scratch now, not in the first run; with
        `queries`, also the tables that depend on their batches' source counts (the prefix
        lengths of the untiled prefix level), so that no run of those groups builds anything."""
        sp = C.c_void_p(stream) if stream else None
        native.check(native.lib().msbfs_solver_prepare(self._h, sp))
        if queries is not None and queries.K:
            native.check(native.lib().msbfs_solver_prepare_queries(
                self._h, queries.K, native.ptr(queries.off, C.c_int64),
                native.ptr(queries.ids, C.c_int32), sp))

    def prepare_hybrid(self, part: int, nparts: int, stream: Optional[int] = None) -> None:
        """prepare() for the hybrid phase A of rank `part` of `nparts` (its own vertices)."""
        native.check(native.lib().msbfs_solver_prepare_hybrid(
            self._h, int(part), int(nparts), C.c_void_p(stream) if stream else None))

    def tune(self, tuning) -> None:
        spec = tuning if isinstance(tuning, str) else ",".join(
            f"{k}={v}" for k, v in dict(tuning).items())
        native.check(native.lib().msbfs_solver_tune(self._h, spec.encode()))

    def run(self, queries: QuerySet, count_edges: bool = False, stream: Optional[int] = None
            ) -> BfsResult:
        K = queries.K
        F = np.zeros(K, dtype=np.int64)
        E = np.zeros(K, dtype=np.int64) if count_edges else None
        st = native.Stats()
        if K:
            native.check(native.lib().msbfs_solver_run(
                self._h, K, native.ptr(queries.off, C.c_int64), native.ptr(queries.ids, C.c_int32),
                native.ptr(F, C.c_int64), native.ptr(E, C.c_int64) if E is not None else None,
                C.byref(st), C.c_void_p(stream) if stream else None))
        return BfsResult(F, None if E is None else E // 2, st.as_dict())

    def distances(self, queries: QuerySet, out_ptr: Optional[int] = None,
                  ld: Optional[int] = None, stream: Optional[int] = None,
                  out: Optional[np.ndarray] = None) -> BfsResult:
        """F plus the per-vertex distances of every group: dist[k, v] = BFS level of vertex v
        (original ids, also on relabelled graphs) from group k, 0 for its valid sources, -1 where
        unreached; dist[k][dist[k] >= 0].sum() == F[k].

        Host output (default): BfsResult.dist is int32[K, n] (a view of the first n columns of
        `out` when given: a C-contiguous int32 [K, ld >= n] array written in place, its columns
        >= n untouched). One solver pass of rows at a time is staged on the device.
        out_ptr: an integer device address of K x ld int32 (ld defaults to n) that receives the
        rows instead; nothing is copied to the host and BfsResult.dist is None."""
        if out_ptr is not None and out is not None:
            raise ValueError("give out_ptr (device) or out (host), not both")
        return self._matrix_run("msbfs_solver_run_dist", queries,
                                None if out_ptr is None else [out_ptr], 1, ld, stream, out)

    def _matrix_run(self, fn: str, queries: QuerySet, ptrs, count: int, ld: Optional[int],
                    stream: Optional[int], out: Optional[np.ndarray] = None) -> BfsResult:
        """distances() / parents(): `count` K x ld int32 matrices through the entry point `fn`,
        into the device addresses `ptrs`, or (ptrs None) through `fn`_host into host matrices
        (the first one `out` when given), returned as their first n columns."""
        K = queries.K
        n = self.graph.n
        F = np.zeros(K, dtype=np.int64)
        st = native.Stats()
        if ptrs is not None:
            ld = n if ld is None else int(ld)
            if ld < n:
                raise ValueError("ld must be at least n")
            args = [C.c_void_p(int(p)) for p in ptrs]
            views = [None] * count
        else:
            D, ld = _host_dist_out(K, n, out, ld)
            hosts = [D] + [np.full((K, ld), -1, dtype=np.int32) for _ in range(count - 1)]
            args = [native.ptr(m, C.c_int32) for m in hosts]
            views = [m[:, :n] for m in hosts]
            fn += "_host"
        if K:
            native.check(getattr(native.lib(), fn)(
                self._h, K, native.ptr(queries.off, C.c_int64), native.ptr(queries.ids, C.c_int32),
                native.ptr(F, C.c_int64), *args, ld, C.byref(st),
                C.c_void_p(stream) if stream else None))
        return BfsResult(F, None, st.as_dict(), *views)

    def parents(self, queries: QuerySet, dist_ptr: Optional[int] = None,
                parent_ptr: Optional[int] = None, ld: Optional[int] = None,
                stream: Optional[int] = None) -> BfsResult:
        """F, the distances (as distances()) and the BFS parents of every group: parent[k, v] = v
        for the valid sources of group k, -1 where unreached, otherwise the first neighbour u of
        v with dist[k, u] == dist[k, v] - 1, "first" in the order of v's row in the device graph
        (graph.download(), internal ids, mapped back through graph.relabel_map()). All device
        solvers return the same matrix on one DeviceGraph; path_to_set / nearest_source read it.

        Host output (default): BfsResult.dist and .parent are int32[K, ld or n][:, :n].
        dist_ptr and parent_ptr: integer device addresses of K x ld int32 each (ld defaults to
        n) that receive the rows instead; BfsResult.dist and .parent are None. One pointer
        without the other raises ValueError."""
        if (dist_ptr is None) != (parent_ptr is None):
            raise ValueError("give both dist_ptr and parent_ptr (device) or neither (host)")
        return self._matrix_run("msbfs_solver_run_parents", queries,
                                None if dist_ptr is None else [dist_ptr, parent_ptr], 2, ld,
                                stream)

    def profile(self, queries: QuerySet, bins=64, stream: Optional[int] = None) -> BfsResult:
        """F exactly as run() returns it plus each group's level profile, at the speed of run():
        .reach[k] = vertices reached (sources included), .ecc[k] = largest distance (-1 for a
        group without a valid source), .hist[k, L] = vertices at distance exactly L for
        L < bins - 1, the last column counting every vertex at distance >= bins - 1. reach and
        ecc are exact whatever `bins` is; hist[k].sum() == reach[k]. bins="all": 64 columns, and
        a second run with max(ecc) + 2 columns if some group gets that far.
        The bit-parallel solver runs the kernels of run() (leaf folding and the device-driven
        level batches included) and keeps the per-level counts it multiplies into F."""
        st = native.Stats()
        sp = C.c_void_p(stream) if stream else None

        def call(F, reach, ecc, hist, nbins):
            native.check(native.lib().msbfs_solver_run_profile(
                self._h, queries.K, native.ptr(queries.off, C.c_int64),
                native.ptr(queries.ids, C.c_int32), native.ptr(F, C.c_int64),
                native.ptr(reach, C.c_int64), native.ptr(ecc, C.c_int32),
                native.ptr(hist, C.c_int64), nbins, nbins, C.byref(st), sp))

        F, reach, ecc, hist = _profile_call(queries.K, bins, call)
        return BfsResult(F, None, st.as_dict(), reach=reach, ecc=ecc, hist=hist)

    def level_trace(self) -> list:
        """Per-level records of the last run / hybrid phase (bit-parallel solver): batch, level,
        dir ('T' push / 'B' pull), kind (which pull a 'B' level ran: 't' tiles, 'p' per-vertex
        prefix, 'h' LDS-hub filtered, 'l' lean + overflow, 'f' full, 'n' plain narrow; '' for a
        push), frontier size nf and degree sum ef entering the level, newly
        visited vertices nf_next, active (bottom-up) or touched (top-down) vertices, host ms."""
        L = native.lib()
        n = int(L.msbfs_solver_levels(self._h, None, 0))
        if n <= 0:
            return []
        buf = (native.Level * n)()
        L.msbfs_solver_levels(self._h, buf, n)
        return [r.as_dict() for r in buf]

    # ---- hybrid multi-GPU mode (parallel/hybrid.py drives these) ----
    def hybrid_max_groups(self) -> int:
        return int(native.lib().msbfs_solver_hybrid_max_groups(self._h))

    def hybrid_phase_a(self, queries: QuerySet, part: int, nparts: int, n_eff: int,
                       count_l1: bool, wbeg: np.ndarray, send_ptr: int,
                       stream: Optional[int] = None, coded: bool = False):
        """Levels 1-2 of all groups, level-2 pulls only for the vertices v = part + i*nparts
        below n_eff; packs their visited words into the device buffer at send_ptr (destination-
        major). Returns (out[2K+3], stats). coded: the send buffer gets one zero-word coded
        segment per destination instead (hybrid.encode_np), stats["coded_len"] their lengths."""
        K = queries.K
        wbeg = np.ascontiguousarray(wbeg, dtype=np.int32)
        out = np.zeros(2 * K + 3, dtype=np.int64)
        st = native.Stats()
        args = (self._h, K, native.ptr(queries.off, C.c_int64), native.ptr(queries.ids, C.c_int32),
                int(part), int(nparts), int(n_eff), int(bool(count_l1)),
                native.ptr(wbeg, C.c_int32), C.c_void_p(send_ptr), native.ptr(out, C.c_int64))
        strm = C.c_void_p(stream) if stream else None
        if coded:
            lens = np.zeros(int(nparts), dtype=np.int64)
            native.check(native.lib().msbfs_solver_hybrid_phase_a_coded(
                *args, native.ptr(lens, C.c_int64), C.byref(st), strm))
            d = st.as_dict()
            d["coded_len"] = lens
            return out, d
        native.check(native.lib().msbfs_solver_hybrid_phase_a(*args, C.byref(st), strm))
        return out, st.as_dict()

    def hybrid_chunk_bounds(self, part: int, nparts: int, n_eff: int, chunks: int) -> np.ndarray:
        """Own-vertex index ranges [b[c], b[c+1]) of a chunked phase A (chunks + 1 entries)."""
        b = np.zeros(int(chunks) + 1, dtype=np.int64)
        native.check(native.lib().msbfs_solver_hybrid_chunk_bounds(
            self._h, int(part), int(nparts), int(n_eff), int(chunks), native.ptr(b, C.c_int64)))
        return b

    def hybrid_phase_a_chunked(self, queries: QuerySet, part: int, nparts: int, n_eff: int,
                               count_l1: bool, wbeg: np.ndarray, send_ptr: int, chunks: int,
                               on_chunk, stream: Optional[int] = None):
        """hybrid_phase_a with the overlapped exchange: after each own-vertex range's words are
        packed (enqueued on the solver's stream), on_chunk(c, i0, i1) is called on this thread
        to start that piece of the all-to-all. Returns (out[2K+3], stats)."""
        K = queries.K
        wbeg = np.ascontiguousarray(wbeg, dtype=np.int32)
        out = np.zeros(2 * K + 3, dtype=np.int64)
        st = native.Stats()
        err = []

        def cb(_user, c, i0, i1):
            if err:
                return
            try:
                on_chunk(int(c), int(i0), int(i1))
            except BaseException as e:  # noqa: BLE001 (re-raised after the native call)
                err.append(e)

        fn = native.ChunkFn(cb)  # (kept alive for the call)
        rc = native.lib().msbfs_solver_hybrid_phase_a_chunked(
            self._h, K, native.ptr(queries.off, C.c_int64), native.ptr(queries.ids, C.c_int32),
            int(part), int(nparts), int(n_eff), int(bool(count_l1)), native.ptr(wbeg, C.c_int32),
            C.c_void_p(send_ptr), native.ptr(out, C.c_int64), int(chunks), fn, None,
            C.byref(st), C.c_void_p(stream) if stream else None)
        if err:
            raise err[0]
        native.check(rc)
        return out, st.as_dict()

    def hybrid_decode(self, coded_ptr: int, coded_len: np.ndarray, nparts: int, n_eff: int,
                      w_count: int, dense_ptr: int, stream: Optional[int] = None) -> None:
        """Expand the received coded segments (coded_len[r] u64 from each part r, back to back)
        into the dense layout hybrid_phase_c reads (asynchronous on the solver's stream)."""
        lens = np.ascontiguousarray(coded_len, dtype=np.int64)
        native.check(native.lib().msbfs_solver_hybrid_decode(
            self._h, C.c_void_p(coded_ptr), native.ptr(lens, C.c_int64), int(nparts), int(n_eff),
            int(w_count), C.c_void_p(dense_ptr), C.c_void_p(stream) if stream else None))

    def hybrid_phase_c(self, K: int, w_begin: int, w_count: int, nparts: int, n_eff: int,
                       recv_ptr: int, reduced: np.ndarray, stream: Optional[int] = None):
        """Levels >= 3 of the groups in words [w_begin, w_begin + w_count) from the exchanged
        words at recv_ptr (per source part, w_count u64 of each of its vertices). Returns
        (F_local[64 * w_count], stats)."""
        reduced = np.ascontiguousarray(reduced, dtype=np.int64)
        if len(reduced) != 2 * K + 3:
            raise ValueError("reduced must have 2K+3 entries")
        F = np.zeros(max(1, 64 * w_count), dtype=np.int64)
        st = native.Stats()
        native.check(native.lib().msbfs_solver_hybrid_phase_c(
            self._h, int(K), int(w_begin), int(w_count), int(nparts), int(n_eff),
            C.c_void_p(recv_ptr), native.ptr(reduced, C.c_int64), native.ptr(F, C.c_int64),
            C.byref(st), C.c_void_p(stream) if stream else None))
        return F, st.as_dict()

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            native.lib().msbfs_solver_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def cpu_bfs(graph: Graph, queries: QuerySet, threads: int = 0, count_edges: bool = False,
            distances: bool = False, out: Optional[np.ndarray] = None,
            parents: bool = False, profile: bool = False, bins=64) -> BfsResult:
    """Query-parallel host BFS (native C++ threads). distances=True: BfsResult.dist is the
    int32[K, n] distance matrix (see Solver.distances; `out` as there). parents=True: the
    distances plus BfsResult.parent, the int32[K, n] BFS parents (see Solver.parents; "first
    neighbour" in the row order of `graph`). profile=True: BfsResult.reach, .ecc and .hist with
    `bins` columns (see Solver.profile); not together with distances or parents."""
    K = queries.K
    if profile:
        if distances or parents:
            raise ValueError("profile=True does not combine with distances or parents")

        def call(F, reach, ecc, hist, nbins):
            native.check(native.lib().msbfs_cpu_run_profile(
                graph.n, native.ptr(graph.rowptr, C.c_int64), native.ptr(graph.col, C.c_int32),
                K, native.ptr(queries.off, C.c_int64), native.ptr(queries.ids, C.c_int32),
                native.ptr(F, C.c_int64), native.ptr(reach, C.c_int64),
                native.ptr(ecc, C.c_int32), native.ptr(hist, C.c_int64), nbins, nbins,
                int(threads)))

        F, reach, ecc, hist = _profile_call(K, bins, call)
        E = None
        if count_edges:
            E = cpu_bfs(graph, queries, threads, count_edges=True).edges
        return BfsResult(F, E, {}, reach=reach, ecc=ecc, hist=hist)
    F = np.zeros(K, dtype=np.int64)
    E = np.zeros(K, dtype=np.int64) if count_edges else None
    if distances or parents:
        D, ld = _host_dist_out(K, graph.n, out, None)
        Pm = np.full((K, ld), -1, dtype=np.int32) if parents else None
        ga = (graph.n, native.ptr(graph.rowptr, C.c_int64), native.ptr(graph.col, C.c_int32), K,
              native.ptr(queries.off, C.c_int64), native.ptr(queries.ids, C.c_int32),
              native.ptr(F, C.c_int64), native.ptr(D, C.c_int32))
        if K and parents:
            native.check(native.lib().msbfs_cpu_run_parents(*ga, native.ptr(Pm, C.c_int32), ld,
                                                            int(threads)))
        elif K:
            native.check(native.lib().msbfs_cpu_run_dist(*ga, ld, int(threads)))
        if E is not None and K:
            deg = np.diff(graph.rowptr)
            E[:] = [int(deg[D[k, :graph.n] >= 0].sum()) // 2 for k in range(K)]
        return BfsResult(F, E, {}, D[:, :graph.n], None if Pm is None else Pm[:, :graph.n])
    if K:
        native.check(native.lib().msbfs_cpu_run(
            graph.n, native.ptr(graph.rowptr, C.c_int64), native.ptr(graph.col, C.c_int32), K,
            native.ptr(queries.off, C.c_int64), native.ptr(queries.ids, C.c_int32),
            native.ptr(F, C.c_int64), native.ptr(E, C.c_int64) if E is not None else None,
            int(threads)))
    return BfsResult(F, E, {})


def multi_source_bfs(graph: Union[Graph, DeviceGraph], queries: QuerySet, algo: str = "auto",
                     device: int = 0, count_edges: bool = False, distances: bool = False,
                     parents: bool = False, profile: bool = False, bins=64,
                     **opts) -> BfsResult:
    """One-shot convenience wrapper (creates and frees a Solver). distances=True: the result
    also carries the int32[K, n] distance matrix (Solver.distances); parents=True: that and the
    BFS parent matrix (Solver.parents); profile=True (not with either): the level profile with
    `bins` columns (Solver.profile). The traversed-edge counts then come from a second, plain
    run when count_edges is set too."""
    if profile and (distances or parents):
        raise ValueError("profile=True does not combine with distances or parents")
    if algo == "cpu":
        if isinstance(graph, DeviceGraph):
            graph = graph.download()
        return cpu_bfs(graph, queries, count_edges=count_edges, distances=distances,
                       parents=parents, profile=profile, bins=bins)
    dg = graph if isinstance(graph, DeviceGraph) else DeviceGraph.from_host(graph, device)
    with Solver(dg, algo, max_groups=max(1, queries.K), **opts) as s:
        if not distances and not parents and not profile:
            return s.run(queries, count_edges=count_edges)
        if profile:
            r = s.profile(queries, bins=bins)
        else:
            r = s.parents(queries) if parents else s.distances(queries)
        if count_edges:
            r.edges = s.run(queries, count_edges=True).edges
        return r


def path_to_set(parent_row: np.ndarray, v: int) -> list:
    """The shortest path [v, ..., source] from v to its group, read off one row of a parent
    matrix (BfsResult.parent[k]); [] if v is unreached. Its length is dist[k, v] + 1."""
    parent_row = np.asarray(parent_row)
    v = int(v)
    if not 0 <= v < len(parent_row) or parent_row[v] < 0:
        return []
    path = [v]
    while int(parent_row[v]) != v:
        v = int(parent_row[v])
        path.append(v)
        if len(path) > len(parent_row):
            raise ValueError("parent_row has a cycle: not a BFS parent array")
    return path


def nearest_source(parent: np.ndarray) -> np.ndarray:
    """int32[K, n]: the source each vertex's parent path ends at (the member of the group it is
    nearest to under the first-in-row rule; the graph Voronoi partition), -1 where unreached.
    Pointer doubling: ceil(log2(longest path)) numpy passes over the matrix."""
    P = np.array(parent, dtype=np.int32, ndmin=2)
    K, n = P.shape
    reached = P >= 0
    cur = np.where(reached, P, np.arange(n, dtype=np.int32)[None, :])
    rows = np.arange(K)[:, None]
    for _ in range(max(1, int(n).bit_length())):
        nxt = cur[rows, cur]
        if np.array_equal(nxt, cur):
            break
        cur = nxt
    out = np.where(reached, cur, -1).astype(np.int32)
    return out if np.ndim(parent) == 2 else out[0]


def harmonic(hist: np.ndarray) -> np.ndarray:
    """Harmonic closeness of every group from its level histogram (BfsResult.hist):
    sum over L >= 1 of hist[:, L] / L, float64[K] (a float for one row). The tail column mixes
    levels, so a non-zero tail of a histogram with more than one column raises ValueError (ask
    for more bins, or bins="all")."""
    H = np.array(hist, dtype=np.int64, ndmin=2)
    nb = H.shape[1]
    if nb > 1 and np.any(H[:, nb - 1] != 0):
        raise ValueError("the tail bucket is not empty: the histogram has too few bins")
    out = (H[:, 1:] / np.arange(1, max(nb, 1), dtype=np.float64)).sum(axis=1) if nb > 1 \
        else np.zeros(H.shape[0], dtype=np.float64)
    return out if np.ndim(hist) == 2 else float(out[0])


def within(hist: np.ndarray, r: int) -> np.ndarray:
    """Vertices within r hops of every group (its sources included) from its level histogram:
    int64[K] (an int for one row). r must lie below the tail column, whose vertices have no
    single distance, unless that column is zero (then every reached vertex is counted)."""
    H = np.array(hist, dtype=np.int64, ndmin=2)
    nb = H.shape[1]
    r = int(r)
    if r < 0:
        out = np.zeros(H.shape[0], dtype=np.int64)
    else:
        if r >= nb - 1 and np.any(H[:, nb - 1] != 0) and nb > 0:
            raise ValueError("r reaches the tail bucket: the histogram has too few bins")
        out = H[:, :min(r, nb - 1) + 1].sum(axis=1)
    return out if np.ndim(hist) == 2 else int(out[0])


def argmin_first(F: np.ndarray) -> int:
    """Reference tie-break (main.cu:381-397): first valid F, strict '<' => lowest index wins.
    Returns -1 for K == 0."""
    F = np.asarray(F)
    valid = np.nonzero(F >= 0)[0]
    if len(valid) == 0:
        return -1
    return int(valid[np.argmin(F[valid])])  # argmin returns the first minimum
