// Bit-parallel MS-BFS: per-vertex distance output. A distance run (RunOutputs::dist) rides
// the edge-counting instantiation, the one mode in which every level leaves a materialised new
// frontier list and an exact new-bit row per frontier vertex; right after each k_count_frontier
// a k_record_levels launch stores the level number for every new (vertex, group) bit into the
// caller's group-major matrix out[group * ld + original vertex id]. Level 0 comes from the
// batch's source pairs (k_record_sources), the -1 fill from a memset of the pass's rows, so
// every (vertex, group) pair is stored exactly once per run: plain stores, no atomics.
#pragma once

#include "common.hpp"

namespace msbfs {
namespace bp {

// What a distance run hands to the level bodies (a member of the solver, set for the run's
// duration; out == nullptr: no distance output, nothing of this file is launched).
struct Record {
  int32_t* out = nullptr;          // row 0 = group 0 of the run
  int64_t ld = 0;                  // row stride (elements), >= n
  int64_t k0 = 0, nb = 0;          // the current batch's groups [k0, k0 + nb)
  const int32_t* new2old = nullptr;  // internal id -> user id (nullptr: the graph keeps its ids)
  int32_t* slot = nullptr;           // n marks of the dense walk (relabelled graphs), all zero
  // a parents run (RunOutputs::parent): the BFS parent matrix, laid out like out, the
  // run's own seen rows and the wide search's queue (below); all nullptr in a plain distance run
  int32_t* parent = nullptr;
  uint64_t* seen = nullptr;
  int32_t* wq = nullptr;    // n entries
  uint32_t* wcnt = nullptr;  // its length, zero between levels
};

// The lane mapping of k_record_levels. Rows of the output lie ld * 4 bytes apart, so the 64 bits
// of one word never share a cache line; what a mapping can choose is which lanes store together.
// Kept: one lane per list entry and a wave-uniform loop over the groups set anywhere in the
// wave's 64 entries, so that the lanes holding a group store into one row and neighbouring ids
// share lines. Measured against the Lay<W> mapping of k_count_frontier (G lanes per vertex, each
// lane walking its own set bits, a wave's stores going to up to 64 rows): equal where the ids
// scatter, 10-28 % less record time where they do not (profiles/distances.md).
//
// On a relabelled graph the list is in internal id order and new2old scatters every store. The
// large levels therefore go through the user's id order instead (dense): k_record_mark leaves
// slot[new2old[u]] = u + 1 for the list's vertices (one scattered store per vertex, not one per
// vertex and group), and the record kernel walks all n user ids, takes the marked ones (clearing
// the mark) and gathers their rows, so its stores fall into shared lines again.

// new bits of v = a[v] (& ~b[v] with DIFF), as in k_count_frontier. fl's length comes from the
// device counter (a closed level of a device-driven batch has none and writes nothing). out:
// row 0 = the batch's first group; only rows below nb are written. slot != nullptr: the dense
// walk over the marks of k_record_mark instead of the list.
template <int W, bool DIFF>
__global__ __launch_bounds__(kBlock) void k_record_levels(const int32_t* fl, const Ctr* ctr,
                                                          const uint64_t* a, const uint64_t* b,
                                                          const int32_t* new2old, int32_t* slot,
                                                          int64_t n, int32_t* out, int64_t ld,
                                                          int64_t nb, int32_t level) {
  const int64_t nf = ctr->fl2.v;
  if (nf == 0) return;
  const int64_t cnt = slot ? n : nf;
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  for (int64_t tb = (int64_t)blockIdx.x * kBlock; tb < cnt; tb += (int64_t)gridDim.x * kBlock) {
    const int64_t idx = tb + wv * 64 + lane;
    int32_t v = -1;
    int64_t o = 0;  // the user's id of v
    if (idx < cnt) {
      if (slot) {
        v = slot[idx] - 1;
        if (v >= 0) slot[idx] = 0;
        o = idx;
      } else {
        v = fl[idx];
      }
    }
    const bool valid = v >= 0 && v < n;
    if (!slot && valid) o = new2old ? new2old[v] : v;
    if (!__ballot(valid)) continue;  // (wave-uniform: a dense tile without a marked id)
    int32_t* col = out + (valid ? o : 0);
#pragma unroll 1
    for (int j = 0; j < W; ++j) {
      uint64_t x = 0;
      if (valid) {
        x = a[(int64_t)v * W + j];
        if constexpr (DIFF) x &= ~b[(int64_t)v * W + j];
      }
      // the groups of word j set on any lane of the wave (wave-uniform, so a scalar loop)
      uint64_t any = x;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) any |= __shfl_xor(any, off);
      any = (uint64_t)uni64((int64_t)any);
      while (any) {
        const int bit = __ffsll((unsigned long long)any) - 1;
        any &= any - 1;
        const int64_t k = (int64_t)j * 64 + bit;
        if (((x >> bit) & 1ull) && k < nb) col[k * ld] = level;
      }
    }
  }
}

// slot[new2old[u]] = u + 1 for the list's vertices (slot is all zero before and after a level)
static __global__ __launch_bounds__(kBlock) void k_record_mark(const int32_t* fl, const Ctr* ctr,
                                                               const int32_t* new2old, int64_t n,
                                                               int32_t* slot) {
  const int64_t nf = ctr->fl2.v;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nf;
       i += (int64_t)gridDim.x * kBlock) {
    const int32_t u = fl[i];
    if (u < 0 || u >= n) continue;
    const int32_t o = new2old[u];
    if (o >= 0 && o < n) slot[o] = u + 1;
  }
}

// the dense walk pays from this share of the vertices on (an n-entry pass per level otherwise)
constexpr int64_t kRecordDenseDiv = 16;

// ---- BFS parents (RunOutputs::parent) -----------------------------------------------------------
// parent[group * ld + user id of v] = user id of the FIRST neighbour u, in the order of v's row
// in the device graph, that group reached one level before v. A parents run is a distance run
// that also owns seen[n * W]: the (vertex, group) bits recorded through the previous level, by
// internal id. It is built only from what k_record_levels consumes (the source pairs, the new
// frontier list and its new-bit rows); the solver's visited rows are inexact in places (lazy
// fills, dskip, alive masks). Per level k_record_parents (and k_record_parents_wide, below)
// searches against the seen rows that entered the level, then k_record_commit ORs the level's
// new bits into them: separate launches, so that no search reads a row the same level already
// committed. A neighbour u of v (level L) with a seen bit of the group has level <= L - 1, and
// >= L - 1 as v's neighbour, so it is a parent; BFS guarantees that every new bit finds one
// before the row ends.
//
// Vertices below kRecordWideDeg: the Lay<W>::G lanes of a vertex walk its row together, each
// lane testing its own words of the neighbour's seen row (one coalesced 8W-byte load), the
// exit group-uniform, kRecordInFlight neighbours in flight per step. From kRecordWideDeg on the
// search only queues the vertex, and k_record_parents_wide, a third launch between search and
// commit, gives each queued vertex a whole block: 1024 row entries per step, the hits of a step
// settled per (word, bit) by the lowest row position (an LDS atomicMin), which keeps the
// first-in-row rule. A hub reached early finds most of its parents far down its degree-sorted
// row: inside the search kernel one wave walked such a row alone, one dependent load after the
// other (RMAT-22, 64 groups: 12.5 ms for level 1), and the hubs of a relabelled graph sit side
// by side in the list, i.e. in the same waves. The bound is a constant, not a tuning key: the
// result does not depend on it. A graph without such a vertex (max_degree below the bound: the
// road-like graphs of the device-driven push batches among them) never launches the wide kernel.
constexpr int kRecordWideDeg = kParentsWideDegree;  // (msbfs/device.hpp)
constexpr int kRecordInFlight = 4;

template <int W, bool DIFF>
__global__ __launch_bounds__(kBlock) void k_record_parents(
    const int32_t* fl, const Ctr* ctr, const uint64_t* a, const uint64_t* b, const int64_t* rowptr,
    const int32_t* col, const uint64_t* seen, const int32_t* new2old, int64_t n, int32_t* parent,
    int64_t ld, int64_t nb, int32_t* wq, uint32_t* wcnt) {
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, VPW = L::VPW, TILE = L::TILE, PB = kRecordInFlight;
  const int64_t nf = ctr->fl2.v;
  if (nf == 0) return;
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  const int wv = threadIdx.x >> 6;
  for (int64_t tb = (int64_t)blockIdx.x * TILE; tb < nf; tb += (int64_t)gridDim.x * TILE) {
    const int64_t idx = tb + wv * VPW + sub;
    int32_t v = -1;
    if (idx < nf) v = fl[idx];
    const bool valid = v >= 0 && v < n;
    V<VW> x = vzero<VW>();  // the still parentless new bits of this lane's words
    int64_t rb = 0, re = 0;
    int32_t ov = 0;  // the user's id of v
    if (valid) {
      const int64_t vo = (int64_t)v * W + slot * VW;
      x = ldv<VW>(a + vo);
      if constexpr (DIFF) {
        const V<VW> o = ldv<VW>(b + vo);
#pragma unroll
        for (int j = 0; j < VW; ++j) x.w[j] &= ~o.w[j];
      }
      ld_rowptr(rowptr, v, rb, re);
      ov = new2old ? new2old[v] : v;
    }
    bool xnz = false;
#pragma unroll
    for (int j = 0; j < VW; ++j) xnz |= x.w[j] != 0;
    bool gopen = ((__ballot(xnz) >> (sub * G)) & L::GBITS) != 0;  // (group-uniform)
    const bool wide = valid && re - rb >= kRecordWideDeg;
    // ---- narrow: the lane group walks the row, PB neighbours per step (whole wave, uniform loop)
    int64_t pos = rb;
    bool open = gopen && !wide && pos < re;
    while (__ballot(open)) {
      int32_t u[PB];
#pragma unroll
      for (int q = 0; q < PB; ++q) {
        u[q] = (open && pos + q < re) ? col[pos + q] : -1;
        if (u[q] >= n) u[q] = -1;
      }
      V<VW> sr[PB];
#pragma unroll
      for (int q = 0; q < PB; ++q) {
        sr[q] = vzero<VW>();
        if (u[q] >= 0) sr[q] = ldv<VW>(seen + (int64_t)u[q] * W + slot * VW);
      }
#pragma unroll
      for (int q = 0; q < PB; ++q) {
        bool hit = false;
#pragma unroll
        for (int j = 0; j < VW; ++j) hit |= (x.w[j] & sr[q].w[j]) != 0;
        if (hit) {
          const int32_t ou = new2old ? new2old[u[q]] : u[q];
#pragma unroll
          for (int j = 0; j < VW; ++j) {
            uint64_t y = x.w[j] & sr[q].w[j];
            x.w[j] &= ~y;
            while (y) {
              const int bit = __ffsll((unsigned long long)y) - 1;
              y &= y - 1;
              const int64_t k = (int64_t)(slot * VW + j) * 64 + bit;
              if (k < nb) parent[k * ld + ov] = ou;
            }
          }
        }
      }
      pos += PB;
      xnz = false;
#pragma unroll
      for (int j = 0; j < VW; ++j) xnz |= x.w[j] != 0;
      const bool still = ((__ballot(xnz) >> (sub * G)) & L::GBITS) != 0;
      open = open && still && pos < re;
    }
    // ---- wide: queued for k_record_parents_wide (at most one entry per list vertex)
    {
      const bool q = wide && gopen && slot == 0;
      const uint32_t at = wave_append(q, wcnt);
      if (q) wq[at] = v;
    }
  }
}

// The queued wide vertices (wq[0, *wcnt): internal ids, each with a new bit), one block per
// vertex and kRecordWideStep row entries per step. best[word * 64 + bit] = the lowest row
// position that hit the still open bit; steps go up the row, so the first step with a hit holds
// the row's first, and a settled bit is closed in xs and never hit again.
constexpr int kRecordWideStep = 4 * kBlock;

template <int W, bool DIFF>
__global__ __launch_bounds__(kBlock) void k_record_parents_wide(
    const int32_t* wq, const uint32_t* wcnt, const uint64_t* a, const uint64_t* b,
    const int64_t* rowptr, const int32_t* col, const uint64_t* seen, const int32_t* new2old,
    int64_t n, int32_t* parent, int64_t ld, int64_t nb) {
  constexpr int U = kRecordWideStep / kBlock;
  __shared__ uint64_t xs[W];
  __shared__ uint32_t best[64 * W];
  const uint32_t cnt = *wcnt;
  const int tid = threadIdx.x;
  for (uint32_t e = blockIdx.x; e < cnt; e += gridDim.x) {
    const int32_t v = wq[e];
    if (v < 0 || v >= n) continue;  // (block-uniform)
    int64_t rb, re;
    ld_rowptr(rowptr, v, rb, re);
    const int32_t ov = new2old ? new2old[v] : v;
    __syncthreads();  // (the previous vertex's last reads of xs / best)
    for (int i = tid; i < 64 * W; i += kBlock) best[i] = ~0u;
    if (tid < W) {
      uint64_t x = a[(int64_t)v * W + tid];
      if constexpr (DIFF) x &= ~b[(int64_t)v * W + tid];
      xs[tid] = x;
    }
    __syncthreads();
    for (int64_t p = rb; p < re; p += kRecordWideStep) {
      uint64_t xl[W];  // (the same on every thread: read between two barriers)
      bool left = false;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        xl[j] = xs[j];
        left |= xl[j] != 0;
      }
      if (!left) break;
      int32_t u[U];
#pragma unroll
      for (int q = 0; q < U; ++q) {
        const int64_t pos = p + q * kBlock + tid;
        u[q] = pos < re ? col[pos] : -1;
        if (u[q] >= n) u[q] = -1;
      }
#pragma unroll
      for (int q = 0; q < U; ++q) {
        if (u[q] < 0) continue;
        const uint32_t off = (uint32_t)(p + q * kBlock + tid - rb);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          if (!xl[j]) continue;
          uint64_t h = seen[(int64_t)u[q] * W + j] & xl[j];
          while (h) {
            const int bit = __ffsll((unsigned long long)h) - 1;
            h &= h - 1;
            atomicMin(&best[j * 64 + bit], off);
          }
        }
      }
      __syncthreads();
      for (int i = tid; i < 64 * W; i += kBlock) {
        const uint32_t bo = best[i];
        if (bo == ~0u || !((xs[i >> 6] >> (i & 63)) & 1ull)) continue;
        const int32_t pu = col[rb + bo];
        if (i < nb) parent[(int64_t)i * ld + ov] = new2old ? new2old[pu] : pu;
        atomicAnd((unsigned long long*)&xs[i >> 6], ~(1ull << (i & 63)));
      }
      __syncthreads();
    }
  }
}

// seen[v] |= the level's new bits of v, for the list's vertices (each listed once): one thread
// per (entry, word), plain read-modify-write. Also empties the wide queue for the next level.
template <int W, bool DIFF>
__global__ __launch_bounds__(kBlock) void k_record_commit(const int32_t* fl, const Ctr* ctr,
                                                          const uint64_t* a, const uint64_t* b,
                                                          int64_t n, uint64_t* seen,
                                                          uint32_t* wcnt) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *wcnt = 0;  // (the level's wide queue is spent)
  const int64_t cnt = (int64_t)ctr->fl2.v * W;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cnt;
       i += (int64_t)gridDim.x * kBlock) {
    const int32_t v = fl[i / W];
    if (v < 0 || v >= n) continue;
    const int64_t o = (int64_t)v * W + (i % W);
    uint64_t x = a[o];
    if constexpr (DIFF) x &= ~b[o];
    if (x) seen[o] |= x;
  }
}

}  // namespace bp
}  // namespace msbfs
