// Bit-parallel MS-BFS: the first pull level's sparse row codes and the tail push of the prefix
// pull (before the pulls, or after the tiled prefix pull).
#pragma once

#include "common.hpp"

namespace msbfs {
namespace bp {

// ---------------------------------------------------------------------------------------------
// Sparse row codes for the first bottom-up level. Its frontier is the level-1 frontier: outside
// the top hubs a vertex there was reached from one or two sources, so its visited row (8*W bytes)
// mostly holds a single set bit (RMAT-26, 1024 groups: ~1.2 bits per row below degree ~9K).
// Gathering those rows made the level bound by Infinity-Cache traffic (rocprofv3, k_bu_chunks at
// level 2: 44 % L2 hit rate, ~115 GB of L2 misses for 0.74e9 row gathers). code[u] (32 bit):
// 0 = row empty; else bits 30-31 = number of set groups c (1-3) and bits 10*i .. 10*i+9 their
// ids (groups < 1024); kDenseCode = anything else (gathered as before). Several slots: the
// multi-bit rows of the mid-degree ids (RMAT-26: degree 1K-8K, 1-2 expected bits) were most of
// the level's L2 misses (the dense rows left did not fit one XCD's 4 MB L2 next to the top hubs'
// rows; single-slot codes 7.5 ms for the level's chunk pulls, two slots 6.9 ms). The
// frontier's codes occupy a 64x smaller footprint than its rows, so the pulls mostly hit L2.
// Only ids >= code_from use codes: after degree relabelling the lower ids are the hubs, whose rows
// are dense and L2-resident. The codes live in the top-down touched buffer (unused by bottom-up
// levels, rebuilt by every top-down level).
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kDenseCode = 0xFFFFFFFFu;  // (3 slots of group 1023: never a real code)
constexpr int kCodeSlots = 3;
// group of slot i of a sparse code, -1 for an unused slot
__device__ __forceinline__ int code_g(uint32_t c, int i) {
  return i < (int)(c >> 30) ? (int)((c >> (10 * i)) & 1023u) : -1;
}
constexpr int32_t kNoCodes = INT32_MAX;

template <int W>
// ids [lo, hi), then the list entries fl[0..nl) >= hi
__global__ __launch_bounds__(kBlock) void k_build_codes(const uint64_t* R, const uint32_t* anyvis,
                                                        int64_t lo, int64_t hi, const int32_t* fl,
                                                        int64_t nl, uint32_t* code) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < hi - lo + nl;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t u = i < hi - lo ? lo + i : (int64_t)fl[i - (hi - lo)];
    if (i >= hi - lo && u < hi) continue;
    uint32_t c = 0;
    if (any_visited(anyvis, (int32_t)u)) {
      int pc = 0;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        uint64_t w = R[u * W + j];
        const int pw = __popcll(w);
        if (pc + pw <= kCodeSlots) {  // (dense hub rows skip the bit loop)
          while (w) {
            const int b = __ffsll((unsigned long long)w) - 1;
            w &= w - 1;
            c |= (uint32_t)(j * 64 + b) << (10 * pc);
            ++pc;
          }
        } else {
          pc += pw;
        }
      }
      c = pc == 0 ? 0u : pc <= kCodeSlots ? c | ((uint32_t)pc << 30) : kDenseCode;
    }
    code[u] = c;
  }
}

// ---------------------------------------------------------------------------------------------
// Prefix pull + tail push for the first bottom-up level (rows sorted by id, degree relabelled).
// The LDS hub bitmap covers the ids < H; a pull that scanned whole rows had to probe the global
// visited bitmap for every neighbour id >= H (the degree tail: ~40 % of the edge endpoints on
// RMAT-26, almost none of them in the level-1 frontier). Instead the pulls stop at the first id
// >= H, and the few level-1 frontier vertices u >= H push their bits to their neighbours here:
// acc[v] |= row(u) (atomicOr, mostly one word thanks to the sparse codes) and stamp[v] = epoch
// (stamp = nullptr: the consumer reads every vertex's acc row instead).
// The narrow pull folds acc[v] of stamped vertices into its accumulator (and clears it); wide
// vertices collect it with their chunk results in k_bu_wide_finalize. Sources need no push:
// every neighbour of a source was reached at level 1. Only own vertices (v % nparts == part) are
// targets (the hybrid mode's level 2 pulls only those), and done vertices are skipped, so every
// written acc entry is consumed and cleared within the level.
// ---------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(kBlock) void k_push_tail(
    const int32_t* fl, int64_t nf, int32_t H, const int64_t* rowptr, const int32_t* col,
    const uint64_t* R, const uint32_t* code, int32_t code_from, const uint32_t* done,
    int part, int nparts, uint64_t* acc, int32_t* stamp, int32_t epoch, int split,
    int32_t vmax = INT32_MAX) {
  constexpr int PG = 64;  // lanes per wave: an entry's lanes take consecutive row entries
  // `split` waves per frontier entry (wave s of entry i takes row entries s*64 + lane, step
  // split*64; the host splits small frontiers only), UN entries per lane in flight: a frontier
  // vertex of degree 30K otherwise kept one wave busy for ~470 dependent rounds of column id ->
  // done probe -> atomic while the rest of the grid had finished (RMAT-30 / 32 groups: ~10K
  // frontier vertices push; 1024 groups: ~100K+, mostly of low degree, one wave each)
  constexpr int UN = 4;
  const int SPLIT = split;
  // own targets: v % nparts == part (hybrid phase A); a power-of-two count tests the low bits
  // instead of dividing (v % nparts: ~40 VALU per neighbour entry)
  const uint32_t pmask = (nparts & (nparts - 1)) == 0 ? (uint32_t)(nparts - 1) : 0u;
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / PG;
  const int64_t nwave = ((int64_t)gridDim.x * kBlock) / PG;
  for (int64_t wi = wave; wi < nf * SPLIT; wi += nwave) {
    const int64_t i = wi / SPLIT;
    const int sp = (int)(wi % SPLIT);
    const int32_t u = fl[i];
    if (u < H) continue;
    const uint32_t c = (code && u >= code_from) ? code[u] : kDenseCode;
    if (c == 0) continue;
    const int64_t b = rowptr[u], e = rowptr[u + 1];
    const int64_t kStep = (int64_t)SPLIT * PG;
    for (int64_t k0 = b + sp * PG + lane; k0 < e; k0 += UN * kStep) {
      int32_t v[UN];
      bool ok[UN];
#pragma unroll
      for (int q = 0; q < UN; ++q) {  // loads first (clamped index), tests after
        const int64_t k = k0 + q * kStep;
        const int32_t x = col[k < e ? k : k0];
        v[q] = x;
        ok[q] = k < e && x < vmax;  // (vmax: leaf folding pushes to no id >= n_core)
      }
#pragma unroll
      for (int q = 0; q < UN; ++q)
        if (nparts > 1)
          ok[q] = ok[q] && (pmask ? ((uint32_t)v[q] & pmask) == (uint32_t)part
                                  : v[q] % nparts == part);
      if (done) {  // (nullptr: the consumer clears done rows too)
        uint32_t dw[UN];
#pragma unroll
        for (int q = 0; q < UN; ++q) dw[q] = done[v[q] >> 5];
#pragma unroll
        for (int q = 0; q < UN; ++q) ok[q] = ok[q] && !((dw[q] >> (v[q] & 31)) & 1u);
      }
#pragma unroll
      for (int q = 0; q < UN; ++q) {
        if (!ok[q]) continue;
        if (c != kDenseCode) {
          for (int s = 0; s < kCodeSlots; ++s) {
            const int g = code_g(c, s);
            if (g >= 0)
              atomicOr((unsigned long long*)&acc[(int64_t)v[q] * W + (g >> 6)], 1ull << (g & 63));
          }
        } else {
          for (int j = 0; j < W; ++j) {
            const uint64_t w = R[(int64_t)u * W + j];
            if (w)
              atomicOr((unsigned long long*)&acc[(int64_t)v[q] * W + j], (unsigned long long)w);
          }
        }
        if (stamp) stamp[v[q]] = epoch;  // (nullptr: the consumer reads every acc row)
      }
    }
  }
}

// The tail push AFTER the tiled prefix pull (tuning key push_after; one GPU, no chunked
// exchange): the pushed bits go straight into the level's output rows O, so the tile epilogue
// reads no acc row (4.2 GB on RMAT-26 / 1024 groups, every tile vertex) and a push whose bit
// the prefix pull already set costs a plain load instead of an atomic. The push then does the
// accounting of what it adds (the epilogue has run): per-group counts of the bits its
// atomicOr newly set (LDS counters -> this block's slab row), and for a vertex it gave its
// first new bit of the level, the frontier bit (+ count, degree sum), and for one it gave its
// first bit at all, the any-visited bit (+ degree sum). A vertex the pushed bits complete is
// left not done (the next pull finds it covered). Census (tools/tail_push_stats.py, RMAT-26):
// 179K tail pushers, 40.7M pushed edges, 42.5M code slots, 6.9M distinct targets.
template <int W>
__global__ __launch_bounds__(kBlock) void k_push_tail_after(
    const int32_t* fl, int64_t nf, int32_t H, const int64_t* rowptr, const int32_t* col,
    const uint64_t* R, const uint32_t* code, int32_t code_from, uint64_t* O, uint32_t* fbm,
    uint32_t* anyvis, Ctr* ctr, uint32_t* slabF, int32_t vmax = INT32_MAX) {
  __shared__ uint32_t cnt[64 * W];
  __shared__ unsigned long long scratch[kWaves];
  __shared__ uint32_t scratch32[kWaves];
  for (int i = threadIdx.x; i < 64 * W; i += kBlock) cnt[i] = 0;
  __syncthreads();
  unsigned long long ef = 0, ev = 0;
  uint32_t nfc = 0;
  const int lane = lane_id();
  const int64_t grp = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int64_t ngrp = ((int64_t)gridDim.x * kBlock) >> 6;
  for (int64_t i = grp; i < nf; i += ngrp) {
    const int32_t u = fl[i];
    if (u < H) continue;
    const uint32_t c = (code && u >= code_from) ? code[u] : kDenseCode;
    if (c == 0) continue;
    const int64_t b = rowptr[u], e = rowptr[u + 1];
    for (int64_t k = b + lane; k < e; k += 64) {
      const int32_t v = col[k];
      if (v >= vmax) continue;  // (leaf folding: an id >= n_core has no output row)
      // (every target has its output row: the tiles and the big vertices' finalize write one
      // for the vertices done before this level too, holding every alive group)
      bool added = false;
      if (c != kDenseCode) {
        for (int s = 0; s < kCodeSlots; ++s) {
          const int g = code_g(c, s);
          if (g < 0) continue;
          unsigned long long* p = (unsigned long long*)&O[(int64_t)v * W + (g >> 6)];
          const unsigned long long bit = 1ull << (g & 63);
          if (*p & bit) continue;  // (set by the pull or an earlier push: bits only get set)
          if (!(atomicOr(p, bit) & bit)) {
            atomicAdd(&cnt[g], 1u);
            added = true;
          }
        }
      } else {
        for (int j = 0; j < W; ++j) {
          const uint64_t w = R[(int64_t)u * W + j];
          if (!w) continue;
          uint64_t nb = w & ~(uint64_t)atomicOr((unsigned long long*)&O[(int64_t)v * W + j],
                                                (unsigned long long)w);
          added |= nb != 0;
          while (nb) {
            atomicAdd(&cnt[j * 64 + __ffsll((unsigned long long)nb) - 1], 1u);
            nb &= nb - 1;
          }
        }
      }
      if (added) {  // (plain loads first: most targets got new bits from the pull already)
        const uint32_t m = 1u << (v & 31);
        const bool in_f = (fbm[v >> 5] & m) != 0, seen = (anyvis[v >> 5] & m) != 0;
        if (!in_f || !seen) {
          const unsigned long long dv = (unsigned long long)(rowptr[v + 1] - rowptr[v]);
          if (!in_f && !(atomicOr(&fbm[v >> 5], m) & m)) {
            ++nfc;
            ef += dv;
          }
          if (!seen && !(atomicOr(&anyvis[v >> 5], m) & m)) ev += dv;
        }
      }
    }
  }
  block_sum_add32(nfc, &ctr->fl2.v, scratch32);
  block_sum_add(ef, &ctr->ef2.v, scratch);
  block_sum_add(ev, &ctr->ev2.v, scratch);
  __syncthreads();
  uint32_t* row = slabF + (size_t)blockIdx.x * (64 * W);
  for (int i = threadIdx.x; i < 64 * W; i += kBlock) row[i] = cnt[i];
}

}  // namespace bp
}  // namespace msbfs
