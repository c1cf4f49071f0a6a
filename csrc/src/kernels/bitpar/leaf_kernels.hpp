// Bit-parallel MS-BFS: the kernels of leaf folding (bitpar/leaf.hpp): the leaf weights of the
// parents, the per-level weighted count of the parents' new bits, and the correction for leaves
// that are sources themselves.
#pragma once

#include "common.hpp"
#include "leaf.hpp"

namespace msbfs {
namespace bp {

// leafw[h] = row entries of h that are >= n_core (sorted rows: the row's tail), h < n_core
static __global__ __launch_bounds__(kBlock) void k_leaf_weights(const int64_t* rowptr,
                                                                const int32_t* col, int64_t n_core,
                                                                int32_t* leafw) {
  for (int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x; h < n_core;
       h += (int64_t)gridDim.x * kBlock) {
    const int64_t b = rowptr[h], e = rowptr[h + 1];
    int64_t lo = b, hi = e;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)col[mid] >= n_core) hi = mid;
      else lo = mid + 1;
    }
    leafw[h] = (int32_t)(e - lo);
  }
}

// What the weighted count reads. It keeps its own record of what it has counted: seen[pi] = the
// bits of the parent at list position pi counted so far in this batch, valid where epoch[pi] is
// the batch's epoch (else all zero: no per-batch fill); epoch[pi] = minus the batch's epoch marks
// a parent that is complete. The new bits of a level are then
//   done parent:  alive & ~seen   (it holds every alive group; its row may be stale or, under
//                                  dskip, not written at the level it finished). It can gain
//                                  nothing after that: marked complete, no row read or written
//   otherwise:    R[h] & ~seen    (R = the buffer the level wrote, current for every vertex
//                                  that is not done; all zero while no group has visited h)
// whatever kind of level ran. alive = the mask the level's own kernels used: new bits lie inside
// it, and a parent marked done under it or an earlier (larger) one holds all of it.
struct LeafArgs {
  const int32_t* plist;
  const int32_t* pw;
  const int32_t* pidx;
  uint64_t* seen;
  int32_t* epoch;
  int32_t batch_epoch;  // in [1, INT32_MAX)
  const uint64_t* R;
  const uint32_t* anyvis;
  const uint32_t* done;
  const uint64_t* alive;
  const uint64_t* gmask;
  unsigned long long* F;
  uint32_t weight;  // level + 1
  Prof prof;        // a profile run: the counts also go to level `weight` of its histogram
};

// parents per lane group and block iteration: the pass is a chain of dependent loads (list
// position -> epoch, done and any-visited bits -> rows), so several are kept in flight
constexpr int kLeafU = 4;

// The new bits of the parents h[u] (list positions pi[u], both valid where ok[u]) on this lane's
// slice, recorded as seen; whole wave, uniform control flow. Loads by stage, each stage's for all
// U parents first.
template <int W>
__device__ __forceinline__ void leaf_new_bits(const LeafArgs& a, const bool (&ok)[kLeafU],
                                              const int32_t (&h)[kLeafU],
                                              const int64_t (&pi)[kLeafU],
                                              const V<Lay<W>::VW>& am,
                                              V<Lay<W>::VW> (&nw)[kLeafU]) {
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, U = kLeafU;
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  int32_t ep[U];
  uint32_t dw[U], aw[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    ep[u] = 0;
    dw[u] = aw[u] = 0u;
    if (ok[u]) {
      ep[u] = a.epoch[pi[u]];
      dw[u] = a.done[h[u] >> 5];
      aw[u] = a.anyvis[h[u] >> 5];
    }
  }
  bool live[U], fin[U];
  V<VW> seen[U], cur[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    live[u] = ok[u] && ep[u] != -a.batch_epoch && ((aw[u] >> (h[u] & 31)) & 1u);
    fin[u] = live[u] && ((dw[u] >> (h[u] & 31)) & 1u);
    seen[u] = vzero<VW>();
    cur[u] = fin[u] ? am : vzero<VW>();
    if (live[u] && ep[u] == a.batch_epoch) seen[u] = ldv<VW>(a.seen + pi[u] * W + slot * VW);
    if (live[u] && !fin[u]) cur[u] = ldv<VW>(a.R + (int64_t)h[u] * W + slot * VW);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      nw[u].w[j] = cur[u].w[j] & ~seen[u].w[j];
      any |= nw[u].w[j] != 0;
    }
    // (the G lanes of a parent store its whole row; they all read the epoch before the store)
    const bool g_any = (__ballot(any) >> (sub * G)) & L::GBITS;
    if (fin[u]) {
      if (slot == 0) a.epoch[pi[u]] = -a.batch_epoch;
    } else if (g_any) {
#pragma unroll
      for (int j = 0; j < VW; ++j) seen[u].w[j] |= nw[u].w[j];
      stv<VW>(a.seen + pi[u] * W + slot * VW, seen[u]);
      if (slot == 0) a.epoch[pi[u]] = a.batch_epoch;
    }
  }
}

// block counters -> F (one atomic per group with a count per block; `cnt` holds weighted counts,
// below 2^31: the leaves of a graph are fewer than that)
template <int W>
__device__ __forceinline__ void leaf_flush(const uint32_t* cnt, const LeafArgs& a) {
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * W; i += kBlock)
    if (cnt[i]) {
      atomicAdd(&a.F[i], (unsigned long long)cnt[i] * a.weight);
      if (a.prof.hist) prof_add(a.prof, 64 * W, i, a.weight, cnt[i]);
    }
}

// The parents of the weight classes 1 .. kLeafClasses: list positions [0, npos), npos a multiple
// of kLeafPad, every tile of one weight (pw of its first position). Register bit-sliced counters,
// multiplied by the weight when they spill.
template <int W>
__global__ __launch_bounds__(kBlock) void k_leaf_weigh(LeafArgs a, int64_t npos) {
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, VPW = L::VPW, TILE = L::TILE, U = kLeafU;
  static_assert(kLeafPad % TILE == 0, "a tile lies in one weight class");
  __shared__ uint32_t cnt[64 * W];
  for (int i = threadIdx.x; i < 64 * W; i += kBlock) cnt[i] = 0;
  __syncthreads();
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  const int wv = threadIdx.x >> 6;
  const V<VW> am = alive_mask<VW>(a.alive, a.gmask, slot);
  BitCounter<VW> bc;
  bc.zero();
  int nadd = 0;
  uint32_t curw = 0;
  auto spill_w = [&] {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      uint64_t any = bc.any(j);
      const int base = (slot * VW + j) * 64;
      while (any) {
        const int b = __ffsll((unsigned long long)any) - 1;
        any &= any - 1;
        atomicAdd(&cnt[base + b], bc.count(j, b) * curw);
      }
    }
    bc.zero();
    nadd = 0;
  };
  for (int64_t tb = (int64_t)blockIdx.x * (U * TILE); tb < npos;
       tb += (int64_t)gridDim.x * (U * TILE)) {
    bool ok[U];
    int32_t h[U];
    int64_t pi[U];
    uint32_t wt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t0 = tb + (int64_t)u * TILE;  // (block-uniform)
      pi[u] = t0 + wv * VPW + sub;
      h[u] = -1;
      wt[u] = 0;
      if (t0 < npos) {  // (npos is a multiple of TILE: the whole tile is inside)
        wt[u] = (uint32_t)a.pw[t0];
        h[u] = a.plist[pi[u]];
      }
      ok[u] = h[u] >= 0;
    }
    V<VW> nw[U];
    leaf_new_bits<W>(a, ok, h, pi, am, nw);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (wt[u] == 0) continue;  // (past the end; block-uniform)
      if (wt[u] != curw || nadd == (1 << BitCounter<VW>::D) - 1) {
        spill_w();
        curw = wt[u];
      }
      bc.add(nw[u]);
      ++nadd;
    }
  }
  spill_w();
  leaf_flush<W>(cnt, a);
}

// Parents of any weight, bit by bit (an LDS add of the weight per new bit): the vertices of
// `list` (n of them, or *n_dev where given) that are parents, or, without a list, the list
// positions [pos0, pos0 + n) (the heavy parents).
template <int W>
__global__ __launch_bounds__(kBlock) void k_leaf_weigh_list(LeafArgs a, const int32_t* list,
                                                            int64_t n_arg, const uint32_t* n_dev,
                                                            int64_t pos0, int32_t n_core) {
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, VPW = L::VPW, TILE = L::TILE, U = kLeafU;
  __shared__ uint32_t cnt[64 * W];
  for (int i = threadIdx.x; i < 64 * W; i += kBlock) cnt[i] = 0;
  __syncthreads();
  const int64_t n = n_dev ? (int64_t)*n_dev : n_arg;
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  const int wv = threadIdx.x >> 6;
  const V<VW> am = alive_mask<VW>(a.alive, a.gmask, slot);
  for (int64_t tb = (int64_t)blockIdx.x * (U * TILE); tb < n;
       tb += (int64_t)gridDim.x * (U * TILE)) {
    bool ok[U];
    int32_t h[U];
    int64_t pi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t idx = tb + (int64_t)u * TILE + wv * VPW + sub;
      h[u] = -1;
      pi[u] = -1;
      if (idx < n) {
        if (list) h[u] = list[idx];
        else pi[u] = pos0 + idx;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (list) pi[u] = (h[u] >= 0 && h[u] < n_core) ? (int64_t)a.pidx[h[u]] : -1;
      else if (pi[u] >= 0) h[u] = a.plist[pi[u]];
      ok[u] = pi[u] >= 0 && h[u] >= 0;
      if (!ok[u]) pi[u] = 0;
    }
    uint32_t lw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) lw[u] = ok[u] ? (uint32_t)a.pw[pi[u]] : 0u;
    V<VW> nw[U];
    leaf_new_bits<W>(a, ok, h, pi, am, nw);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        uint64_t x = nw[u].w[j];
        const int base = (slot * VW + j) * 64;
        while (x) {
          const int b = __ffsll((unsigned long long)x) - 1;
          x &= x - 1;
          atomicAdd(&cnt[base + b], lw[u]);
        }
      }
  }
  leaf_flush<W>(cnt, a);
}

// Leaves that are sources (right after k_init; first[i] = pair i is the first (vertex, group)
// pair of its kind, from k_init's atomicOr). vis = the rows after k_init: bit g of p's row says
// that p is a source of g (read through anyvis: only sources are marked yet, and a lazy batch's
// other rows are stale). F is unsigned and wraps; the batch's sum is right at its end. A profile
// run moves the same leaves between the levels of its histogram (k_init counted every source at
// level 0): out of level 1 where p is a source, out of level 2 where it is not; the other end of
// a two-vertex component comes in at level 1.
template <int W>
__global__ __launch_bounds__(kBlock) void k_leaf_sources(const int32_t* pv, const int32_t* pk,
                                                         const uint8_t* first, int64_t np,
                                                         const int32_t* relabel,
                                                         const int64_t* rowptr, const int32_t* col,
                                                         const uint64_t* vis,
                                                         const uint32_t* anyvis, int32_t n_core,
                                                         int32_t n_eff, unsigned long long* F,
                                                         Prof prof = Prof{}) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < np;
       i += (int64_t)gridDim.x * kBlock) {
    if (!first[i]) continue;
    int32_t v = pv[i];
    if (relabel) v = relabel[v];
    if (v < n_core || v >= n_eff) continue;
    const int k = pk[i];
    const int32_t p = col[rowptr[v]];
    const bool psrc =
        any_visited(anyvis, p) && ((vis[(int64_t)p * W + (k >> 6)] >> (k & 63)) & 1ull);
    if (p < n_core) {
      atomicAdd(&F[k], 0ull - (psrc ? 1ull : 2ull));
      if (prof.hist) atomicAdd(&prof.hist[(size_t)(psrc ? 1 : 2) * (64 * W) + k], 0ull - 1ull);
    } else if (!psrc) {
      atomicAdd(&F[k], 1ull);
      if (prof.hist) atomicAdd(&prof.hist[(size_t)(64 * W) + k], 1ull);
    }
  }
}

}  // namespace bp
}  // namespace msbfs
