// Bit-parallel MS-BFS: per-vertex distance output. A distance run (BitparSolver::run_dist) rides
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

}  // namespace bp
}  // namespace msbfs
