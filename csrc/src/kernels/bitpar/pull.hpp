// Bit-parallel MS-BFS: bottom-up (pull) level kernels — the narrow lane-group pull, the lean
// first-row pass, hub edge chunks and the wide finalize. The list kernels: pull_lists.hpp; sparse
// row codes and the tail push: pull_tail.hpp.
#pragma once

#include "common.hpp"
#include "pull_lists.hpp"
#include "pull_plan.hpp"
#include "pull_tail.hpp"

namespace msbfs {
namespace bp {

// ---------------------------------------------------------------------------------------------
// bottom-up, narrow vertices: G lanes per vertex, early exit when every alive group is covered.
// Each step takes C = 8 neighbours: the group's G lanes load and filter them cooperatively
// (8/G column ids + 8/G bitmap probes per lane instead of 8 + 8), then every lane pulls its
// slot of each surviving neighbour's row (ids broadcast inside the group by shuffles).
// A variant is one config type (below, named after the plan's kinds) with the members:
// BT = block size; HUBW > 0: probes of the HUBW*32 lowest ids (hubs) read an LDS snapshot of
// the visited bitmap (see k_bu_chunks; big blocks amortise the copy).
// ---------------------------------------------------------------------------------------------
//
// FUSE: the level's new-bit counts are accumulated here (register bit-sliced counters -> LDS ->
// this block's row of the counter slab, slabF = first row of this launch) instead of by a
// separate k_count_frontier pass that re-reads both rows of every new frontier vertex.
// PFX (prefix-pull level, see k_push_tail): rows are scanned only over their prefix plen[v] (the
// ids below the level's bound H <= HUBW*32, see BitparSolver::pfx_bound),
// and pushed bits (acc of vertices with stamp == epoch; every vertex's acc when stamp is
// nullptr) seed the accumulator.
// CS = neighbours per step (rows gathered between two coverage checks).
// C1 > 0 (unfiltered levels only): a first step of just C1 rows before the CS-wide steps; late
// levels are mostly covered by the first neighbour or two (sorted rows: hubs first).
// FBM: the new frontier goes into the bitmap fbm (passed as fl2) and its size into ctr->fl2, no
// frontier list (the prefix level at few words, whose next level pulls: see level_bu).
// MINW = waves per SIMD the launch bounds ask for.
struct NarrowBase {  // the plain filtered 256-thread pull; the variants override what differs
  static constexpr int BT = kBlock, HUBW = 0, CS = 8, C1 = 0, MINW = 4;
  static constexpr bool FILT = true, PFX = false, FBM = false;
};
// the prefix level (PullKind::Prefix). 4-neighbour steps when fused: 122 VGPRs, no spills
// (8-neighbour steps spilled at the 128-VGPR bound): RMAT-26 5.17 -> 4.96 ms (the full pulls of
// level 3 keep 8: 5.8 vs 6.8 ms); FBM: frontier bitmap in place of the list (PullPlan::fbm_out)
template <int W, bool FUSE_>
struct NarrowPrefix : NarrowBase {
  static constexpr bool FUSE = FUSE_, PFX = true, FBM = FUSE_;
  static constexpr int BT = pfx_block(W), HUBW = kHubW, CS = FUSE_ ? 4 : 8,
                       MINW = FUSE_ ? pfx_minw(W) : 4;
};
template <bool FUSE_>
struct NarrowHub : NarrowBase {  // PullKind::Hub, the small LDS hub bitmap
  static constexpr bool FUSE = FUSE_;
  static constexpr int BT = 1024, HUBW = kHubW;
};
template <bool FUSE_>
struct NarrowHubBig : NarrowBase {  // PullKind::Hub with PullPlan::hub_big
  static constexpr bool FUSE = FUSE_;
  static constexpr int BT = 1024, HUBW = kHubBig;
};
template <bool FUSE_>
struct NarrowFiltered : NarrowBase {  // PullKind::Narrow with PullPlan::filter
  static constexpr bool FUSE = FUSE_;
};
template <bool FUSE_>
struct NarrowPlain : NarrowBase {  // PullKind::Narrow, no probes
  static constexpr bool FUSE = FUSE_, FILT = false;
};
// 8-row steps after a 1-row first step: PullPlan::short1, the lean pass's overflow list and the
// device-driven batches (all fused: an edge-counting run takes none of them)
template <bool FUSE_>
struct NarrowShort1 : NarrowBase {
  static constexpr bool FUSE = FUSE_, FILT = false;
  static constexpr int C1 = 1;
};

template <int W, class Cfg>
__global__ __launch_bounds__(Cfg::BT, Cfg::MINW) void k_bu_narrow(
    const int32_t* act, int64_t nact, const int64_t* rowptr, const int32_t* col,
    const uint64_t* R, uint64_t* Wb, const uint64_t* alive, const uint64_t* gmask, uint32_t* done,
    int32_t* act2, int32_t* fl2, Ctr* ctr, uint32_t* anyvis, int32_t filter_from, int32_t* actw2,
    int next_wide, uint32_t* slabF, uint64_t* pacc, const int32_t* stamp, int32_t epoch,
    const int32_t* plen, const uint32_t* nact_dev, const uint32_t* snap, BuGate gate) {
  constexpr int BT = Cfg::BT, HUBW = Cfg::HUBW, CS = Cfg::CS, C1 = Cfg::C1;
  constexpr bool FUSE = Cfg::FUSE, FILT = Cfg::FILT, PFX = Cfg::PFX, FBM = Cfg::FBM;
  static_assert(!PFX || HUBW > 0, "the prefix pull relies on the LDS hub bitmap");
  if (!bu_gate_open(gate)) return;  // closed level of a device-driven batch (uniform)
  // snap (first pull level of a batch that did not clear its visited buffer, see start_batch):
  // the any-visited bitmap as of the level start. Probes read it (a vertex first visited during
  // this level may still have a stale row) and an own row it does not mark is all zero.
  const uint32_t* pvis = snap ? snap : anyvis;
  if (nact_dev) nact = (int64_t)*nact_dev;  // (list length known only on the device)
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, VPW = L::VPW;
  // done / any-visited bits: one atomic per word of the wave (wave_set_bits) where a wave
  // holds many vertices or many first visits (W = 16 levels 3-4 measured ~0.4 ms slower each)
  constexpr bool kCombine = G <= 4 || PFX;
  constexpr int NWV = BT / 64, TILE = NWV * VPW;
  constexpr int C = CS;                      // neighbours per step
  constexpr int Q = C / G > 0 ? C / G : 1;   // ids loaded per lane per step
  static_assert(G * Q == C || (C < G && Q == 1), "step = whole lane groups or part of one");
  __shared__ LdsQueue qa, qf, qw;
  __shared__ unsigned long long scratch[NWV];
  __shared__ uint32_t hub[HUBW > 0 ? HUBW : 1];
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  const int wv = threadIdx.x >> 6;
  // counter rows bank-skewed (65, see spill_strided) except on the prefix level: its sparse
  // spills ran level 2 ~0.2 ms slower skewed (4 runs each); 5 slices there, 6 elsewhere
  using Counts = GroupCounts<W, PFX ? 5 : 6, PFX ? 64 : 65, false>;
  __shared__ uint32_t cnt[FUSE ? Counts::kLdsWords : 1];
  Counts gc(cnt, slot);
  if constexpr (HUBW > 0)
    for (int i = threadIdx.x; i < HUBW; i += BT) hub[i] = pvis[i];
  if constexpr (FUSE) gc.zero(BT);
  q_init(qa);
  q_init(qf);
  q_init(qw);
  __syncthreads();
  // (written out, not alive_mask: the helper costs the fused hub variant at 4 words 2 spills)
  V<VW> am;
#pragma unroll
  for (int j = 0; j < VW; ++j) am.w[j] = alive[slot * VW + j] & gmask[slot * VW + j];
  unsigned long long eu = 0, ef = 0, ev = 0;
  uint32_t nfc = 0;  // FBM: new frontier vertices
  __shared__ uint32_t scratch32[FBM ? NWV : 1];
  // Software pipeline over the grid-stride tiles: the active-list entry is loaded two tiles
  // ahead and the vertex's visited row and row offsets one tile ahead, so a tile starts with
  // its column loads instead of two dependent round trips (list entry -> row / offsets).
  const int64_t stride = (int64_t)gridDim.x * TILE, lofs = wv * VPW + sub;
  int64_t tb = (int64_t)blockIdx.x * TILE;
  int32_t v1 = 0, v2 = 0;  // list entries of tiles tb and tb + stride
  V<VW> r1 = vzero<VW>();  // row of v1
  int64_t b1 = 0;          // row offsets of v1
  uint32_t d1 = 0;
  if (tb + lofs < nact) v1 = act[tb + lofs];
  if (tb + stride + lofs < nact) v2 = act[tb + stride + lofs];
  uint32_t p1 = 0;  // PFX: prefix length of v1's row (ids < H)
  if (tb + lofs < nact) {
    r1 = own_row<VW>(R, snap, v1, (int64_t)v1 * W + slot * VW);
    b1 = rowptr[v1];
    d1 = (uint32_t)(rowptr[v1 + 1] - b1);
    if constexpr (PFX) p1 = (uint32_t)plen[v1];
  }
  // one lane per vertex, four-entry steps: aligned 16-byte id loads (col4_aligned, pull_full.hpp)
  constexpr bool A4 = G == 1 && Q == 4 && C == 4;
  int32_t u1[Q];  // first-step column ids of the current tile's vertex (third pipeline stage)
  auto first_ids = [&](bool ok, int32_t (&u)[Q]) {
    if constexpr (A4) {
      const int64_t n1 = ok ? (int64_t)(PFX ? p1 : d1) : 0;
      col4_aligned(col, ok ? b1 : 0, ok ? b1 + n1 : 0, u);
    } else {
#pragma unroll
      for (int q = 0; q < Q; ++q)
        u[q] = (ok && q * G + slot < C && (uint32_t)(q * G + slot) < (PFX ? p1 : d1))
                   ? col[b1 + q * G + slot] : -1;
    }
  };
  first_ids(tb + lofs < nact, u1);
  for (; tb < nact; tb += stride) {
    const int64_t idx = tb + lofs;
    const bool valid = idx < nact;
    const int32_t v = valid ? v1 : 0;
    const V<VW> r = r1;
    const int64_t beg = b1, end = b1 + (PFX ? p1 : d1);  // PFX: pull only the prefix
    const uint32_t deg = d1;
    int32_t u0[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) u0[q] = u1[q];
    // prefetch: row / offsets of the next tile, list entry of the one after
    v1 = v2;
    if (idx + stride < nact) {
      r1 = own_row<VW>(R, snap, v1, (int64_t)v1 * W + slot * VW);
      b1 = rowptr[v1];
      d1 = (uint32_t)(rowptr[v1 + 1] - b1);
      if constexpr (PFX) p1 = (uint32_t)plen[v1];
    }
    if (idx + 2 * stride < nact) v2 = act[idx + 2 * stride];
    V<VW> unv = vzero<VW>(), acc = vzero<VW>();
    bool lane_open = false;
    if (valid) {
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        unv.w[j] = ~r.w[j] & am.w[j];
        lane_open |= unv.w[j] != 0;
      }
    }
    if constexpr (PFX) {  // bits pushed from the tail frontier (k_push_tail)
      if (!stamp) {  // (uniform) no stamps: every vertex reads its row, clears it if set
        const V<VW> a0 = ldv<VW>(pacc + (int64_t)(valid ? v : 0) * W + slot * VW);
        bool set = false;
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          acc.w[j] = valid ? a0.w[j] : 0ull;
          set |= acc.w[j] != 0;
        }
        if (set) stv<VW>(pacc + (int64_t)v * W + slot * VW, vzero<VW>());
      } else if (valid && stamp[v] == epoch) {
        acc = ldv<VW>(pacc + (int64_t)v * W + slot * VW);
        stv<VW>(pacc + (int64_t)v * W + slot * VW, vzero<VW>());
      }
    }
    const bool g_open = valid && ((__ballot(lane_open) >> (sub * G)) & L::GBITS);
    int64_t e0 = beg;
    bool g_cov = false;
    if constexpr (C1 > 0) {
      static_assert(!FILT, "the short first step skips the filter");
      if (g_open) {
        V<VW> x[C1];
#pragma unroll
        for (int c = 0; c < C1; ++c) {
          const int32_t uc = G == 1 ? u0[c] : __shfl(u0[c / G], sub * G + (c % G));
          x[c] = uc >= 0 ? ldv<VW>(R + (int64_t)uc * W + slot * VW) : vzero<VW>();
        }
        bool cov = true;
#pragma unroll
        for (int j = 0; j < VW; ++j) {
#pragma unroll
          for (int c = 0; c < C1; ++c) acc.w[j] |= x[c].w[j];
          cov &= (acc.w[j] & unv.w[j]) == unv.w[j];
        }
        g_cov = !((__ballot(!cov) >> (sub * G)) & L::GBITS);
        e0 = beg + C1;
      }
    }
    if (g_open && !g_cov) {
      for (int64_t e = e0; e < end; e += C) {
        int32_t u[Q];
        bool loaded = false;
        if constexpr (A4) {
          if (!(C1 == 0 && e == beg)) {
            col4_aligned(col, e, end, u);
            loaded = true;
          }
        }
        if (!loaded) {
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            const int64_t ee = e + q * G + slot;
            // first step: preloaded (without the short first step)
            u[q] = (C1 == 0 && e == beg) ? u0[q]
                                         : ((q * G + slot < C && ee < end) ? col[ee] : -1);
          }
        }

        // ids below filter_from are loaded without a probe (filter off: filter_from = INT_MAX)
        // probes: every load first, every use after (with the use next to the load inside the
        // branch the compiler waited for each probe before issuing the next)
        if (FILT && filter_from != INT32_MAX) {  // wave-uniform
          // (LDS and global results in separate registers: a shared destination made the LDS
          // read wait for the outstanding global probes)
          uint32_t pg[Q], ph[Q];
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            pg[q] = ~0u;
            if (u[q] >= filter_from && !(HUBW > 0 && u[q] < HUBW * 32)) pg[q] = pvis[u[q] >> 5];
          }
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            ph[q] = ~0u;
            if (HUBW > 0 && u[q] >= filter_from && u[q] < HUBW * 32) ph[q] = hub[u[q] >> 5];
          }
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (!(((pg[q] & ph[q]) >> (u[q] & 31)) & 1u)) u[q] = -1;
        }
        V<VW> x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          // candidate c = column entry e + c: lane (c % G) of this group holds it in u[c / G]
          const int32_t uc = G == 1 ? u[c] : __shfl(u[c / G], sub * G + (c % G));
          x[c] = uc >= 0 ? ldv<VW>(R + (int64_t)uc * W + slot * VW) : vzero<VW>();
        }
        bool cov = true;
#pragma unroll
        for (int j = 0; j < VW; ++j) {
#pragma unroll
          for (int c = 0; c < C; ++c) acc.w[j] |= x[c].w[j];
          cov &= (acc.w[j] & unv.w[j]) == unv.w[j];
        }
        // the whole group runs this loop in lock step (same v); exit when all lanes covered
        if (!((__ballot(!cov) >> (sub * G)) & L::GBITS)) break;

      }
    }
    const NewBits<VW> nb = gained(r, acc, unv);  // (unv is zero on lanes without a vertex)
    // also when nothing is open: Wb may hold the previous batch's rows
    if (valid) stv<VW>(Wb + (int64_t)v * W + slot * VW, nb.nv);
    if constexpr (FUSE) gc.add(nb.nw);
    const auto [keep, app, g_nf] =
        settle_vertex<W, kCombine>(valid, v, deg, nb, done, anyvis, eu, ef, ev);
    // third stage: the next tile's first-step ids (its offsets arrived during this tile)
    first_ids(idx + stride < nact, u1);
    q_push(qa, keep && (int)deg <= next_wide, v);
    q_push(qw, keep && (int)deg > next_wide, v);
    if constexpr (FBM) {
      wave_set_bits<true>(reinterpret_cast<uint32_t*>(fl2), v, app);
      nfc += app ? 1u : 0u;
      q_flush_n<kQCap, 2>({&qa, &qw}, {act2, actw2}, {&ctr->act2.v, &ctr->actw2.v}, TILE, false);
    } else {
      q_push(qf, app, v);
      q_flush_n<kQCap, 3>({&qa, &qw, &qf}, {act2, actw2, fl2},
                          {&ctr->act2.v, &ctr->actw2.v, &ctr->fl2.v}, TILE, false);
    }
  }
  if constexpr (FBM) {
    q_flush_n<kQCap, 2>({&qa, &qw}, {act2, actw2}, {&ctr->act2.v, &ctr->actw2.v}, 0, true);
    block_sum_add32(nfc, &ctr->fl2.v, scratch32);
  } else {
    q_flush_n<kQCap, 3>({&qa, &qw, &qf}, {act2, actw2, fl2},
                        {&ctr->act2.v, &ctr->actw2.v, &ctr->fl2.v}, 0, true);
  }
  block_sum_add(eu, &ctr->eu2.v, scratch);
  block_sum_add(ef, &ctr->ef2.v, scratch);
  block_sum_add(ev, &ctr->ev2.v, scratch);
  if constexpr (FUSE) gc.store(slabF, BT);
}

// ---------------------------------------------------------------------------------------------
// Late pull levels, first pass: from the third bottom-up level on almost every
// active vertex is covered by its first neighbour (rows sorted: the biggest hub first), and the
// level is bound by the latency of its dependent loads (list entry -> row offsets -> first column
// id -> neighbour row). This lean kernel (no multi-step loop, no software pipeline) keeps few
// registers, so twice as many waves hide that latency. A vertex the first row covers is
// finished here exactly as k_bu_narrow would (row, counts, done bit, frontier, anyvis); the others
// go to an overflow list (ctr->touched, unused by pull levels) that k_bu_narrow then processes
// from scratch.
// ---------------------------------------------------------------------------------------------
// dsnap / skip (tuning dskip, see k_bu_full): a first neighbour done at the level start
// covers every alive group (probe instead of its row); every vertex this pass finishes is done,
// so with skip it writes no row at all.
template <int W>
__global__ __launch_bounds__(kBlock, W >= 16 ? 8 : 6) void k_bu_first(
    const int32_t* act, int64_t nact, const int64_t* rowptr, const int32_t* col,
    const uint64_t* R, uint64_t* Wb, const uint64_t* alive, const uint64_t* gmask, uint32_t* done,
    int32_t* ovf, int32_t* fl2, Ctr* ctr, uint32_t* anyvis, uint32_t* slabF, const int32_t* first,
    const uint32_t* dsnap, int flags) {
  const bool skip = flags & kFlagSkipRows;
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, VPW = L::VPW, TILE = L::TILE;
  // done / any-visited bits: one atomic per word of the wave (wave_set_bits) where a wave
  // holds many vertices or many first visits (W = 16 levels 3-4 measured ~0.4 ms slower each)
  constexpr bool kCombine = G <= 4;
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  const int wv = threadIdx.x >> 6;
  // bank-skewed counter rows (see spill_strided), 32-bit halves (see spill_strided32)
  using Counts = GroupCounts<W, 6, 65, true>;
  __shared__ LdsQueue qo, qf;
  __shared__ unsigned long long scratch[kWaves];
  __shared__ uint32_t cnt[Counts::kLdsWords];
  Counts gc(cnt, slot);
  gc.zero(kBlock);
  q_init(qo);
  q_init(qf);
  __syncthreads();
  const V<VW> am = alive_mask<VW>(alive, gmask, slot);
  unsigned long long ef = 0, ev = 0;
  for (int64_t tb = (int64_t)blockIdx.x * TILE; tb < nact; tb += (int64_t)gridDim.x * TILE) {
    const int64_t idx = tb + wv * VPW + sub;
    const bool valid = idx < nact;
    int32_t v = 0;
    V<VW> r = vzero<VW>(), nw = vzero<VW>();
    uint32_t deg = 0;
    bool open = false, rnz = false;
    if (valid) {
      v = act[idx];
      const int32_t u = first ? first[v] : col[rowptr[v]];  // active vertices have deg > 0
      V<VW> x;
      r = ldv<VW>(R + (int64_t)v * W + slot * VW);
      {
        int64_t b, e;
        ld_rowptr(rowptr, v, b, e);
        deg = (uint32_t)(e - b);  // only counted, off the load chain
      }
      if (dsnap && ((dsnap[u >> 5] >> (u & 31)) & 1u)) x = am;  // (a done first neighbour)
      else x = ldv<VW>(R + (int64_t)u * W + slot * VW);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const uint64_t unv = ~r.w[j] & am.w[j];
        nw.w[j] = x.w[j] & unv;
        open |= (unv & ~nw.w[j]) != 0;
        rnz |= r.w[j] != 0;
      }
    }
    const bool g_open = (__ballot(open) >> (sub * G)) & L::GBITS;
    const bool fin = valid && !g_open;  // covered by the first row: finished at this level
    if (!fin) nw = vzero<VW>();
    if (fin && !skip) {
      V<VW> nv;
#pragma unroll
      for (int j = 0; j < VW; ++j) nv.w[j] = r.w[j] | nw.w[j];
      stv<VW>(Wb + (int64_t)v * W + slot * VW, nv);
    }
    gc.add(nw);
    // (own epilogue: the done bit follows the first-row coverage `fin`, not the new bits)
    bool anynew = false;
#pragma unroll
    for (int j = 0; j < VW; ++j) anynew |= nw.w[j] != 0;
    const bool g_new = (__ballot(anynew) >> (sub * G)) & L::GBITS;
    const bool g_first = g_new && !((__ballot(rnz) >> (sub * G)) & L::GBITS);
    const bool leader = valid && slot == 0;
    wave_set_bits<kCombine>(done, v, leader && fin);
    if (leader && g_new) ef += deg;
    wave_set_bits<kCombine>(anyvis, v, leader && g_first);
    if (leader && g_first) ev += deg;
    q_push(qo, leader && !fin, v);
    q_push(qf, leader && g_new, v);
    q_flush(qo, ovf, &ctr->touched.v, TILE, false);
    q_flush(qf, fl2, &ctr->fl2.v, TILE, false);
  }
  q_flush(qo, ovf, &ctr->touched.v, 0, true);
  q_flush(qf, fl2, &ctr->fl2.v, 0, true);
  block_sum_add(ef, &ctr->ef2.v, scratch);
  block_sum_add(ev, &ctr->ev2.v, scratch);
  gc.store(slabF, kBlock);
}

// bottom-up, wide vertices, phase 1: one wave per edge chunk (<= kChunk edges), processed in
// tiles of 256 edges so the dependent loads are batched instead of chained per neighbour:
//   A) all 64 lanes load 4 column ids each (one coalesced 1-KB pass), optionally test them
//      against the visited-by-anyone bitmap (256 independent loads), and compact the survivors
//      into an LDS list (ballot + popcount prefix);
//   B) the S = 64/G lane groups pull 4 neighbour rows each per step (4*S rows in flight per
//      wave), OR-reduce across groups (xor shuffles) and stop once every alive group is covered.
// The chunk's new bits are merged into acc[v] with atomicOr (k_bu_wide_finalize folds them in).
// offs = inclusive prefix of chunk counts over the wide list.
//
// HUBW > 0 (levels that filter): the block first copies the visited bitmap of the HUBW*32
// lowest ids into LDS. After degree relabelling those are the hubs, which carry most edge
// endpoints (RMAT-26: the top 2^19 ids take roughly two thirds), so most filter probes become
// LDS reads instead of divergent global loads. The copy is a snapshot taken at kernel start; a
// bit another kernel of this level sets later belongs to a vertex first visited at this level,
// whose row in R is still zero, so skipping it is exact. Big blocks (BT threads, 2 per CU)
// amortise the copy; the grid is persistent (grid-stride over chunks).
// One wave pulls edges [beg, lim) of wide vertex v (a chunk) and publishes the new bits into
// acc[v] (k_bu_wide_finalize folds them in). coop: chunks of one vertex run concurrently and
// share progress through acc (see below); coop = 0 (first bottom-up level) skips that.
template <int W, int T, int HUBW>
__device__ __forceinline__ void chunk_pull(int32_t v, int64_t beg, int64_t lim, const int32_t* col,
                                           const uint64_t* R, const V<Lay<W>::VW>& am,
                                           uint64_t* acc, const uint32_t* anyvis,
                                           const uint32_t* hub, int32_t filter_from, int coop,
                                           int32_t* lst, const uint32_t* code,
                                           int32_t code_from, unsigned long long* wacc,
                                           const uint32_t* snap, const uint32_t* dsnap) {
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, S = L::VPW;
  constexpr int PB = VW == 2 ? 4 : 8;  // rows in flight per lane group in phase B
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  const int64_t vo = (int64_t)v * W + slot * VW;
  const V<VW> r = own_row<VW>(R, snap, v, vo);  // see k_bu_narrow
  // g = bits the vertex's other chunks have published so far. Chunks of one hub run
  // concurrently, so each tile publishes its partial OR with a RETURNING atomicOr that also
  // hands back the current union from the memory side (atomics bypass the non-coherent per-XCD
  // L2s); every chunk stops once the union covers all alive groups.
  V<VW> g = vzero<VW>();
  if (coop) {
    if (sub == 0) {
#pragma unroll
      for (int j = 0; j < VW; ++j) g.w[j] = atomicOr((unsigned long long*)&acc[vo + j], 0ull);
    }
#pragma unroll
    for (int j = 0; j < VW; ++j) g.w[j] = __shfl(g.w[j], slot);  // lane slot of sub-group 0
  }
  V<VW> unv, a = vzero<VW>();
  bool lane_open = false;
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    unv.w[j] = ~r.w[j] & am.w[j];
    lane_open |= (unv.w[j] & ~g.w[j]) != 0;
  }
  if (!__ballot(lane_open)) return;  // wave-uniform
  bool covered = false;
  // each: OR the S lane groups' partial rows together and test coverage after every step of
  // PB*S rows; otherwise once per tile. Without early exit across chunks (coop = 0: the first
  // pull level, where hardly any row gets covered) the per-step reduction (3 x VW xor-shuffles)
  // was most of the kernel's LDS instructions: RMAT-26 level-2 chunk pulls 6.63 -> 6.41 ms.
  const bool each = coop != 0;
  for (int64_t t0 = beg; t0 < lim && !covered; t0 += T) {
    // ---- phase A: ids of this tile, filtered, compacted into lst[0..cnt)
    constexpr int Q = T / 64;
    int32_t u[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int64_t e = t0 + q * 64 + lane;
      u[q] = e < lim ? col[e] : -1;
    }
    if (filter_from != INT32_MAX) {
      // probes: every load first, every use after (see k_bu_narrow)
      uint32_t pg[Q], ph[Q];  // separate destinations (see k_bu_narrow)
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        pg[q] = ~0u;
        if (u[q] >= filter_from && !(HUBW > 0 && u[q] < HUBW * 32)) pg[q] = anyvis[u[q] >> 5];
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        ph[q] = ~0u;
        if (HUBW > 0 && u[q] >= 0 && u[q] < HUBW * 32) ph[q] = hub[u[q] >> 5];
      }
#pragma unroll
      for (int q = 0; q < Q; ++q)
        if (u[q] >= 0 && !(((pg[q] & ph[q]) >> (u[q] & 31)) & 1u)) u[q] = -1;
    }
    if (dsnap) {  // (uniform) done neighbours: the alive mask instead of their rows (k_bu_full)
      bool hit = false;
#pragma unroll
      for (int q = 0; q < Q; ++q)
        if (u[q] >= 0 && ((dsnap[u[q] >> 5] >> (u[q] & 31)) & 1u)) {
          u[q] = -1;
          hit = true;
        }
      if (__ballot(hit))
#pragma unroll
        for (int j = 0; j < VW; ++j) a.w[j] |= am.w[j];
    }
    if (code_from != kNoCodes) {  // wave-uniform
      // single-group neighbours: their bit goes into this wave's LDS words (ds_or_b64) instead
      // of a row gather; the words are folded into every lane group's accumulator below
      if (lane < W) wacc[lane] = 0;
      __builtin_amdgcn_wave_barrier();
      uint32_t cd[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        cd[q] = kDenseCode;
        if (u[q] >= code_from) cd[q] = code[u[q]];
      }
#pragma unroll
      for (int q = 0; q < Q; ++q)
        if (cd[q] != kDenseCode) {
#pragma unroll
          for (int i = 0; i < kCodeSlots; ++i) {
            const int g = code_g(cd[q], i);
            if (g >= 0) atomicOr(&wacc[g >> 6], 1ull << (g & 63));
          }
          u[q] = -1;
        }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < VW; ++j) a.w[j] |= wacc[slot * VW + j];
    }
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const uint64_t m = __ballot(u[q] >= 0);
      if (u[q] >= 0) lst[cnt + __popcll(m & lanemask_lt())] = u[q];
      cnt += __popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
    // ---- phase B: rows of the surviving neighbours, PB per lane group per step
    for (int b = 0; b < cnt; b += PB * S) {
      gather_rows<W, PB, false>(lst, cnt, b, R, a);
      if (each) {
        or_across_groups<VW, G>(a);
        if (covers(a, g, unv)) {
          covered = true;
          break;
        }
      }
    }
    if (!each) {  // one cross-group OR and coverage check per tile (see `each`)
      or_across_groups<VW, G>(a);
      if (covers(a, g, unv)) covered = true;
    }
    __builtin_amdgcn_wave_barrier();  // lst is rewritten by the next tile
    // publish this chunk's bits so far and pick up the other chunks' (one round trip)
    if (coop && !covered && t0 + T < lim) {
      bool cov = true;
      if (sub == 0) {
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          const uint64_t nb = a.w[j] & unv.w[j] & ~g.w[j];
          g.w[j] |= nb ? atomicOr((unsigned long long*)&acc[vo + j], nb)
                       : atomicOr((unsigned long long*)&acc[vo + j], 0ull);
          g.w[j] |= nb;
          cov &= ((a.w[j] | g.w[j]) & unv.w[j]) == unv.w[j];
        }
      }
      if (!__ballot(!cov)) covered = true;
#pragma unroll
      for (int j = 0; j < VW; ++j) g.w[j] = __shfl(g.w[j], slot);
    }
  }
  if (sub == 0) {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const uint64_t nb = a.w[j] & unv.w[j] & ~g.w[j];
      if (nb) atomicOr((unsigned long long*)&acc[vo + j], nb);
    }
  }
}

// chunk_pull for the prefix-pull level without codes (fewer than 8 words, or codes off): every
// id of a row prefix is below the LDS hub bitmap's bound, so the probes are LDS reads only, and
// no chunk exits early (coop = 0 at the first pull level). The next tile's column ids are loaded
// while the current tile is probed and gathered; every load is unconditional (clamped index,
// result selected after), so the compiler waits for exactly the loads each use needs instead of
// all of them (RMAT-30 / 32 groups: the level's chunk pulls stream ~10^10 prefix entries at one
// word per vertex, and a wave otherwise waited for every tile's ids from HBM in turn).
template <int W, int T, int HUBW>
__device__ __forceinline__ void chunk_pull_pfx(int32_t v, int64_t beg, int64_t lim,
                                               const int32_t* col, const uint64_t* R,
                                               const V<Lay<W>::VW>& am, uint64_t* acc,
                                               const uint32_t* hub, int32_t* lst,
                                               const uint32_t* snap) {
  static_assert(HUBW > 0, "the prefix chunks probe the LDS hub bitmap");
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, S = L::VPW;
  constexpr int PB = VW == 2 ? 4 : 8;  // rows in flight per lane group in phase B
  constexpr int Q = T / 64;
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  const int64_t vo = (int64_t)v * W + slot * VW;
  // (written out, not own_row: the helper costs this kernel 2 VGPRs)
  const V<VW> r = (snap && !any_visited(snap, v)) ? vzero<VW>() : ldv<VW>(R + vo);
  V<VW> unv, a = vzero<VW>();
  bool lane_open = false;
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    unv.w[j] = ~r.w[j] & am.w[j];
    lane_open |= unv.w[j] != 0;
  }
  if (!__ballot(lane_open)) return;  // wave-uniform
  // ids of the tile at t0 (16-byte aligned): lane l takes entries t0 + 4l .. t0 + 4l + 3 with
  // one aligned 16-byte load (a quarter of the address work of four 4-byte loads; a window past
  // the chunk reads the chunk's first one instead, and an aligned window holding a valid entry
  // never leaves its page), entries outside [beg, lim) are -1
  static_assert(Q == 4, "one 16-byte window per lane");
  typedef int32_t i4 __attribute__((ext_vector_type(4)));
  const int64_t a0 = beg & ~(int64_t)3;
  auto load_ids = [&](int64_t t0, int32_t (&u)[Q]) {
    const int64_t e = t0 + 4 * lane;
    const i4 w = *(const i4*)(col + (e < lim ? e : a0));
    const int32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < Q; ++q) u[q] = (e + q >= beg && e + q < lim) ? x[q] : -1;
  };
  int32_t un[Q];
  load_ids(a0, un);
  bool covered = false;
  for (int64_t t0 = a0; t0 < lim && !covered; t0 += T) {
    int32_t u[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) u[q] = un[q];
    load_ids(t0 + T, un);  // (past the end: clamped, unused)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const uint32_t h = hub[(u[q] >= 0 ? u[q] : 0) >> 5];
      if (u[q] >= 0 && !((h >> (u[q] & 31)) & 1u)) u[q] = -1;
    }
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const uint64_t m = __ballot(u[q] >= 0);
      if (u[q] >= 0) lst[cnt + __popcll(m & lanemask_lt())] = u[q];
      cnt += __popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
    // (unconditional LDS reads from a clamped index, as every load of this pull)
    for (int b = 0; b < cnt; b += PB * S) gather_rows<W, PB, true>(lst, cnt, b, R, a);
    // one cross-group OR and coverage check per tile
    or_across_groups<VW, G>(a);
    if (covers(a, vzero<VW>(), unv)) covered = true;
    __builtin_amdgcn_wave_barrier();  // lst is rewritten by the next tile
  }
  if (sub == 0) {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const uint64_t nb = a.w[j] & unv.w[j];
      if (nb) atomicOr((unsigned long long*)&acc[vo + j], nb);
    }
  }
}

// PFXL: the chunks of a prefix-pull level without codes (chunk_pull_pfx)
template <int W, int T, int BT, int HUBW, bool PFXL = false>
__global__ __launch_bounds__(BT, (BT >= 1024 && HUBW <= 16384) ? 8 : 4) void k_bu_chunks(
    const ChunkDesc* __restrict__ desc, const int64_t* nchunks_p, const int32_t* col,
    const uint64_t* R,
    const uint64_t* alive, const uint64_t* gmask, uint64_t* acc, const uint32_t* anyvis,
    int32_t filter_from, int coop, const uint32_t* code, int32_t code_from,
    const uint32_t* snap, const uint32_t* dsnap = nullptr) {
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G;
  __shared__ int32_t tile[BT / 64][T];
  __shared__ unsigned long long wacc[BT / 64][W];
  __shared__ uint32_t hub[HUBW > 0 ? HUBW : 1];
  if (snap) anyvis = snap;  // probes read the level-start bitmap (see k_bu_narrow)
  if constexpr (HUBW > 0) {
    for (int i = threadIdx.x; i < HUBW; i += BT) hub[i] = anyvis[i];
    __syncthreads();
  }
  const int slot = lane_id() % G;
  int32_t* lst = tile[threadIdx.x >> 6];
  const int64_t nchunks = uni64(*nchunks_p);  // inclusive chunk prefix of the last wide vertex
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const V<VW> am = alive_mask<VW>(alive, gmask, slot);
  // Chunk order. Without early exit (coop = 0: the first bottom-up level, where hardly any row
  // is covered) chunks are dealt round robin over the waves, which balances the hubs' expensive
  // chunks. With early exit a wave takes a contiguous run, so a vertex's later chunks usually
  // come after its earlier ones have published their bits and are skipped at the first check.
  const int64_t cstart = uni64(coop ? nchunks * wave / nwaves : wave);
  const int64_t cend = uni64(coop ? nchunks * (wave + 1) / nwaves : nchunks);
  const int64_t cstep = uni64(coop ? 1 : nwaves);
  ChunkDesc d{0, 0, 0, 0};
  if (cstart < cend) d = desc[cstart];
  for (int64_t c = cstart; c < cend; c += cstep) {
    const int32_t v = uni32(d.v);
    const int64_t beg = uni64((int64_t)(((uint64_t)d.beg_hi << 32) | d.beg_lo));
    const int64_t lim = beg + uni32(d.len);
    if (c + cstep < cend) d = desc[c + cstep];  // next descriptor, in flight during the pull
    if constexpr (PFXL)
      chunk_pull_pfx<W, T, HUBW>(v, beg, lim, col, R, am, acc, hub, lst, snap);
    else
      chunk_pull<W, T, HUBW>(v, beg, lim, col, R, am, acc, anyvis, hub, filter_from, coop,
                             lst, code, code_from, wacc[threadIdx.x >> 6], snap, dsnap);
  }
}

// bottom-up, wide vertices, phase 2: G lanes per vertex fold acc[v] into the visited words.
template <int W, bool FUSE, bool FLB = false>
__global__ __launch_bounds__(kBlock) void k_bu_wide_finalize(
    const int32_t* wl, int64_t nw, const int64_t* rowptr, const uint64_t* R, uint64_t* Wb,
    uint64_t* acc, const uint64_t* alive, const uint64_t* gmask, uint32_t* done, int32_t* actw2,
    int32_t* fl2, Ctr* ctr, uint32_t* anyvis, int32_t* act2n, int next_wide, uint32_t* slabF,
    const uint32_t* snap, uint32_t* fbm = nullptr) {
  // fbm != nullptr (the tiled first pull level, see tiles.hpp): wl is the static big-vertex list,
  // so done vertices are skipped; no list queues: the new frontier goes into bitmap fbm and its
  // size into ctr->fl2, the next active lists come from k_build_active after the level.
  // FLB (with fbm, the narrow pull's FBM levels): wl is the level's wide active list; only the
  // frontier goes into fbm, the next active lists are built here as without fbm.
  using L = Lay<W>;
  constexpr int VW = L::VW, G = L::G, VPW = L::VPW, TILE = L::TILE;
  // done / any-visited bits: one atomic per word of the wave (wave_set_bits) where a wave
  // holds many vertices or many first visits (W = 16 levels 3-4 measured ~0.4 ms slower each)
  constexpr bool kCombine = G <= 4;
  __shared__ LdsQueue qa, qf, qn;
  __shared__ unsigned long long scratch[kWaves];
  const int lane = lane_id(), slot = lane % G, sub = lane / G;
  const int wv = threadIdx.x >> 6;
  // bank-skewed counter rows (see spill_strided): wide vertices gain many groups at once, so
  // every spill touches most counters
  using Counts = GroupCounts<W, 6, 65, false>;
  __shared__ uint32_t cnt[FUSE ? Counts::kLdsWords : 1];
  Counts gc(cnt, slot);
  if constexpr (FUSE) gc.zero(kBlock);
  q_init(qa);
  q_init(qf);
  q_init(qn);
  __syncthreads();
  const V<VW> am = alive_mask<VW>(alive, gmask, slot);
  unsigned long long eu = 0, ef = 0, ev = 0;
  uint32_t nfc = 0;
  __shared__ uint32_t scratch32[kWaves];
  for (int64_t tb = (int64_t)blockIdx.x * TILE; tb < nw; tb += (int64_t)gridDim.x * TILE) {
    const int64_t idx = tb + wv * VPW + sub;
    bool valid = idx < nw;
    int32_t v = 0;
    NewBits<VW> nb{vzero<VW>(), vzero<VW>(), false, false, false};
    uint32_t deg = 0;
    if (valid) {
      v = wl[idx];
      if (fbm && !FLB && is_done(done, v)) {
        // (the tiled level's tail push also pushes into done vertices: leave their acc row clean;
        // and give them their unchanged row in Wb, which k_push_tail_after filters against)
        const int64_t vo = (int64_t)v * W + slot * VW;
        stv<VW>(acc + vo, vzero<VW>());
        stv<VW>(Wb + vo, ldv<VW>(R + vo));
        valid = false;
      }
    }
    if (valid) {
      const int64_t vo = (int64_t)v * W + slot * VW;
      const V<VW> r = own_row<VW>(R, snap, v, vo);
      const V<VW> a = ldv<VW>(acc + vo);
      nb = new_bits(r, a, am);
      stv<VW>(acc + vo, vzero<VW>());
      stv<VW>(Wb + vo, nb.nv);
      deg = (uint32_t)(rowptr[v + 1] - rowptr[v]);
    }
    if constexpr (FUSE) gc.add(nb.nw);  // (zero for invalid lanes)
    const auto [keep, app, g_nf] =
        settle_vertex<W, kCombine>(valid, v, deg, nb, done, anyvis, eu, ef, ev, !fbm || FLB);
    if (fbm) {  // (uniform)
      wave_set_bits<kCombine>(fbm, v, app);
      nfc += app ? 1u : 0u;
      if (!FLB) continue;
    } else {
      q_push(qf, app, v);
    }
    q_push(qa, keep && (int)deg > next_wide, v);
    q_push(qn, keep && (int)deg <= next_wide, v);
    q_flush_n<kQCap, 3>({&qa, &qn, &qf}, {actw2, act2n, fl2},
                        {&ctr->actw2.v, &ctr->act2.v, &ctr->fl2.v}, TILE, false);
  }
  q_flush_n<kQCap, 3>({&qa, &qn, &qf}, {actw2, act2n, fl2},
                      {&ctr->actw2.v, &ctr->act2.v, &ctr->fl2.v}, 0, true);
  if (fbm) block_sum_add32(nfc, &ctr->fl2.v, scratch32);
  block_sum_add(eu, &ctr->eu2.v, scratch);
  block_sum_add(ef, &ctr->ef2.v, scratch);
  block_sum_add(ev, &ctr->ev2.v, scratch);
  if constexpr (FUSE) gc.store(slabF, kBlock);
}

}  // namespace bp
}  // namespace msbfs
