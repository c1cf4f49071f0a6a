// Bit-parallel MS-BFS: bottom-up (pull) levels, the list kernels — active lists, degree bounds,
// row prefix lengths, first neighbours, the wide vertices' chunk descriptors and the seed of a
// device-driven batch.
#pragma once

#include "common.hpp"

namespace msbfs {
namespace bp {

// build the bottom-up active lists (deg > 0, not done) over the vertices v = part + i*nparts,
// i < cnt, split by degree, or by the row prefix length plen[v] when given (the untiled prefix
// level pulls only the prefix: a vertex of high degree with a short prefix is a narrow one)
// (nparts = 1: every vertex; the hybrid mode's vertex-partitioned level pulls only for its own
// residue class)
template <int QCAP>
__global__ __launch_bounds__(kBlock) void k_build_active(int64_t cnt, int part, int nparts,
                                                         const int64_t* rowptr,
                                                         const uint32_t* done, int wide_deg,
                                                         int32_t* act, int32_t* actw, Ctr* ctr,
                                                         const int32_t* plen = nullptr,
                                                         int64_t n_eff = -1) {
  // n_eff >= 0 (with plen, degree-relabelled rows: exactly the vertices < n_eff have edges): no
  // row offsets are read at all (RMAT-30: 8.6 GB), and eu2 stays 0 (its caller reads only the
  // list sizes)
  // Each block owns QCAP consecutive list positions j and flushes its narrow queue once at the
  // end (one counter atomic per QCAP vertices: atomics on one address serialise, and 64K of them
  // were most of this kernel's time on 33M vertices). Blocks are dispatched in order, so the
  // lists come out nearly ascending (hubs first in the wide list: the chunk kernel deals chunks
  // in list order, and a grid-stride build that interleaved distant ranges cost ~1 ms of level-2
  // tail on RMAT-26). The rare wide vertices go through a small queue flushed when needed.
  constexpr int VPT = 4;  // vertices per thread per step (loads first, pushes after)
  constexpr int64_t kStep = (int64_t)VPT * kBlock;
  static_assert(QCAP % kStep == 0, "whole steps per block");
  __shared__ LdsQueueN<QCAP> qn;
  __shared__ LdsQueue qw;
  __shared__ unsigned long long scratch[kWaves];
  q_init(qn);
  q_init(qw);
  __syncthreads();
  unsigned long long eu = 0;
  const int64_t b0 = (int64_t)blockIdx.x * QCAP, b1 = min(b0 + (int64_t)QCAP, cnt);
  for (int64_t b = b0; b < b1; b += kStep) {
    int64_t d[VPT], sd[VPT];
    uint32_t dw[VPT];
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int64_t j = b + q * kBlock + threadIdx.x;
      const int64_t i = part + j * nparts;
      d[q] = 0;
      sd[q] = 0;
      dw[q] = ~0u;
      if (j < b1) {
        if (n_eff >= 0) {
          d[q] = i < n_eff ? 1 : 0;
          if (i < n_eff) sd[q] = (int64_t)plen[i];
        } else {
          d[q] = rowptr[i + 1] - rowptr[i];
          sd[q] = plen ? (int64_t)plen[i] : d[q];
        }
        dw[q] = done[i >> 5];
      }
    }
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int64_t i = part + (b + q * kBlock + threadIdx.x) * nparts;
      const bool ok = d[q] > 0 && !((dw[q] >> (i & 31)) & 1u);
      if (ok && n_eff < 0) eu += (unsigned long long)d[q];
      q_push(qn, ok && sd[q] <= wide_deg, (int32_t)i);
      q_push(qw, ok && sd[q] > wide_deg, (int32_t)i);
    }
    q_flush(qw, actw, &ctr->actw2.v, (int)kStep, false);
  }
  q_flush(qn, act, &ctr->act2.v, 0, true);
  q_flush(qw, actw, &ctr->actw2.v, 0, true);
  block_sum_add(eu, &ctr->eu2.v, scratch);
}

// first id with degree < 2^k for k = 0..kDegBounds-1 (rows relabelled by descending degree: one
// binary search per k, one thread each)
constexpr int kDegBounds = 41;
static __global__ void k_degree_bounds(const int64_t* rowptr, int64_t n, int32_t* out) {
  const int k = threadIdx.x;
  if (k >= kDegBounds) return;
  const int64_t min_deg = (int64_t)1 << k;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid + 1] - rowptr[mid] < min_deg) hi = mid;
    else lo = mid + 1;
  }
  out[k] = (int32_t)lo;
}

// number of vertices with degree > d (bounds the wide list of any pull level)
static __global__ __launch_bounds__(kBlock) void k_count_wide(const int64_t* rowptr, int64_t n, int64_t d,
                                                       unsigned long long* out) {
  __shared__ unsigned long long scratch[kWaves];
  unsigned long long c = 0;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n;
       v += (int64_t)gridDim.x * kBlock)
    c += rowptr[v + 1] - rowptr[v] > d;
  block_sum_add(c, out, scratch);
}

// Chunk descriptor: vertex, first column position, edge count (<= kChunk). Built once per level
// by k_chunk_desc; a wave reads its next descriptor with one scalar load while it pulls the
// current chunk (vs an owner -> list entry -> row offsets chain of dependent loads per chunk).
struct ChunkDesc {
  int32_t v;
  uint32_t beg_lo, beg_hi;
  int32_t len;
};

// first position in the sorted row [b, e) whose id is >= H
__device__ __forceinline__ int64_t row_lower_bound(const int32_t* col, int64_t b, int64_t e,
                                                   int32_t H) {
  while (b < e) {
    const int64_t mid = (b + e) >> 1;
    if (col[mid] < H) b = mid + 1;
    else e = mid;
  }
  return b;
}

// plen[v] = length of v's row prefix with ids < H (rows sorted; a graph property, computed once
// per graph and bound H, see BitparSolver::prefix_lens)
static __global__ __launch_bounds__(kBlock) void k_prefix_lens(const int64_t* rowptr, const int32_t* col,
                                                        int64_t n, int32_t H, int32_t* plen) {
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n;
       v += (int64_t)gridDim.x * kBlock) {
    const int64_t b = rowptr[v];
    plen[v] = (int32_t)(row_lower_bound(col, b, rowptr[v + 1], H) - b);
  }
}

// first[v] = v's first neighbour (rows sorted: after degree relabelling its biggest hub), -1 for
// an isolated vertex: the lean first-row pass (k_bu_first) reads it with one coalesced 4-byte load
// instead of the rowptr -> col chain, whose col[rowptr[v]] touches one 128-byte line per vertex
static __global__ __launch_bounds__(kBlock) void k_first_nbr(const int64_t* rowptr, const int32_t* col,
                                                      int64_t n, int32_t* first) {
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n;
       v += (int64_t)gridDim.x * kBlock) {
    const int64_t b = rowptr[v];
    first[v] = rowptr[v + 1] > b ? col[b] : -1;
  }
}

// chunk counts of the wide vertices' row prefixes (inclusive-scanned into offs by the host)
static __global__ __launch_bounds__(kBlock) void k_prefix_chunks(const int32_t* wl, int64_t nw,
                                                          const int32_t* plen, int64_t* cnt) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nw;
       i += (int64_t)gridDim.x * kBlock)
    cnt[i] = ((int64_t)plen[wl[i]] + kChunk - 1) / kChunk;
}

// plen != nullptr: chunks cover only the row prefixes with ids < H (prefix-pull level)
static __global__ __launch_bounds__(kBlock) void k_chunk_desc(const int32_t* wl, int64_t nw,
                                                       const int64_t* offs, const int64_t* rowptr,
                                                       const int32_t* plen, ChunkDesc* desc) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nw;
       i += (int64_t)gridDim.x * kBlock) {
    const int32_t v = wl[i];
    const int64_t b = rowptr[v];
    const int64_t e = plen ? b + plen[v] : rowptr[v + 1];
    const int64_t c0 = i ? offs[i - 1] : 0, c1 = offs[i];
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t cb = b + (c - c0) * kChunk;
      desc[c] = ChunkDesc{v, (uint32_t)cb, (uint32_t)((uint64_t)cb >> 32),
                          (int32_t)min((int64_t)kChunk, e - cb)};
    }
  }
}

// Two-pass chunk scheduling on the early-exit levels (tuning key chunk2): pass 1 pulls only the
// first chunk of every wide vertex (most are covered by the hubs at the head of their sorted
// rows), pass 2 only the remaining chunks of the vertices pass 1 left open. In one pass every
// chunk of a covered vertex still cost its wave an own-row load and a returning atomic before
// it could skip (RMAT-26 level 3: 313K wide vertices, ~1M+ chunks, 0.5 ms).
static __global__ __launch_bounds__(kBlock) void k_chunk_first(const int32_t* wl, int64_t nw,
                                                               const int64_t* rowptr,
                                                               ChunkDesc* desc, int64_t* cnt) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nw;
       i += (int64_t)gridDim.x * kBlock) {
    const int32_t v = wl[i];
    const int64_t b = rowptr[v], e = rowptr[v + 1];
    desc[i] = ChunkDesc{v, (uint32_t)b, (uint32_t)((uint64_t)b >> 32),
                        (int32_t)min((int64_t)kChunk, e - b)};
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *cnt = nw;
}
// chunks left of wide vertex i after pass 1: 0 once acc[v] (the union its chunks published)
// covers every alive group v misses, else all but the first (G lanes per vertex)
template <int W>
__global__ __launch_bounds__(kBlock) void k_chunk_rest_count(
    const int32_t* wl, int64_t nw, const int64_t* rowptr, const uint64_t* R, const uint64_t* acc,
    const uint64_t* alive, const uint64_t* gmask, const uint32_t* snap, int64_t* cnt) {
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, VPW = L::VPW, TILE = L::TILE;
  const int lane = lane_id(), slot = lane % G, sub = lane / G, wv = threadIdx.x >> 6;
  const V<VW> am = alive_mask<VW>(alive, gmask, slot);
  for (int64_t tb = (int64_t)blockIdx.x * TILE; tb < nw; tb += (int64_t)gridDim.x * TILE) {
    const int64_t i = tb + wv * VPW + sub;
    bool open = false;
    int32_t v = 0;
    if (i < nw) {
      v = wl[i];
      const int64_t vo = (int64_t)v * W + slot * VW;
      const V<VW> r = own_row<VW>(R, snap, v, vo);
      const V<VW> a = ldv<VW>(acc + vo);
#pragma unroll
      for (int j = 0; j < VW; ++j) open |= (~r.w[j] & am.w[j] & ~a.w[j]) != 0;
    }
    const bool g_open = (__ballot(open) >> (sub * G)) & L::GBITS;
    if (i < nw && slot == 0) {
      const int64_t d = rowptr[v + 1] - rowptr[v];
      const int64_t nc = (d + kChunk - 1) / kChunk;
      cnt[i] = g_open && nc > 1 ? nc - 1 : 0;
    }
  }
}
// descriptors of the pass-2 chunks (offs = inclusive prefix of k_chunk_rest_count)
static __global__ __launch_bounds__(kBlock) void k_chunk_rest_desc(const int32_t* wl, int64_t nw,
                                                                   const int64_t* offs,
                                                                   const int64_t* rowptr,
                                                                   ChunkDesc* desc) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nw;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t c0 = i ? offs[i - 1] : 0, c1 = offs[i];
    if (c0 == c1) continue;
    const int32_t v = wl[i];
    const int64_t b = rowptr[v], e = rowptr[v + 1];
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t cb = b + (1 + c - c0) * kChunk;
      desc[c] = ChunkDesc{v, (uint32_t)cb, (uint32_t)((uint64_t)cb >> 32),
                          (int32_t)min((int64_t)kChunk, e - cb)};
    }
  }
}

// counter slot 0 and alive mask 0 of a device-driven pull batch (bu_batch): the host's view
// after the level before the batch
static __global__ void k_bu_seed(Ctr* c0, uint32_t nf, unsigned long long ef, uint32_t nact,
                          uint32_t nactw, unsigned long long eu, const uint64_t* alive,
                          uint64_t* alive0) {
  if (threadIdx.x == 0) {
    c0->fl2.v = nf;
    c0->ef2.v = ef;
    c0->act2.v = nact;
    c0->actw2.v = nactw;
    c0->eu2.v = eu;
  }
  if (threadIdx.x < 16) alive0[threadIdx.x] = alive[threadIdx.x];
}

}  // namespace bp
}  // namespace msbfs
