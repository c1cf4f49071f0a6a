// Bit-parallel MS-BFS solver: bottom-up (pull) levels — active lists, sparse row codes, prefix
// pull + tail push on the first pull level, narrow / lean / hub-chunk pulls after it
// (level_bu). Design overview: bitpar/solver.hpp; kernels: bitpar/pull.hpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "bitpar/init.hpp"
#include "bitpar/leaf_kernels.hpp"
#include "bitpar/pull.hpp"
#include "bitpar/pull_full.hpp"
#include "bitpar/solver.hpp"

namespace msbfs {
namespace bp {

// plen[v] = row prefix length with ids < H for every vertex (cached per graph buffers and H)
const int32_t* BitparSolver::prefix_lens(int32_t H, hipStream_t s) {
  if (plen_key_[0] != (const void*)g_.rowptr || plen_key_[1] != (const void*)g_.col ||
      plen_h_ != H) {
    plen_.ensure((size_t)std::max<int64_t>(g_.n, 1) * sizeof(int32_t));
    k_prefix_lens<<<grid_for(g_.n, kBlock, 8192), kBlock, 0, s>>>(g_.rowptr, g_.col, g_.n, H,
                                                                   plen_.as<int32_t>());
    MSBFS_HIP_CHECK(hipGetLastError());
    plen_key_[0] = g_.rowptr;
    plen_key_[1] = g_.col;
    plen_h_ = H;
    ++plen_builds_;
  }
  return plen_.as<int32_t>();
}

// first[v] for every vertex (cached per graph buffers like prefix_lens); nullptr when the 4n
// bytes do not fit comfortably (RMAT-30): k_bu_first then reads col[rowptr[v]]
const int32_t* BitparSolver::first_nbr(hipStream_t s) {
  if (!first_ok_) return nullptr;
  if (first_key_[0] != (const void*)g_.rowptr || first_key_[1] != (const void*)g_.col) {
    const size_t bytes = (size_t)std::max<int64_t>(g_.n, 1) * sizeof(int32_t);
    if (first_.bytes < bytes) {
      size_t fr = 0, tot = 0;
      MSBFS_HIP_CHECK(hipMemGetInfo(&fr, &tot));
      if (fr < bytes + ((size_t)2 << 30)) {
        first_ok_ = false;
        return nullptr;
      }
    }
    first_.ensure(bytes);
    k_first_nbr<<<grid_for(g_.n, kBlock, 8192), kBlock, 0, s>>>(g_.rowptr, g_.col, g_.n,
                                                                 first_.as<int32_t>());
    MSBFS_HIP_CHECK(hipGetLastError());
    first_key_[0] = g_.rowptr;
    first_key_[1] = g_.col;
  }
  return first_.as<int32_t>();
}

// first id with degree < min_deg (rounded up to a power of two; one table per graph); 0 when
// the graph keeps the user's ids (no degree order to exploit)
int32_t BitparSolver::code_bound(double min_deg) {
  if (!g_.old2new) return 0;
  if (code_key_[0] != (const void*)g_.rowptr || code_key_[1] != (const void*)g_.col ||
      deg_bounds_.empty()) {
    DevBuf b;
    b.alloc(kDegBounds * sizeof(int32_t));
    k_degree_bounds<<<1, 64>>>(g_.rowptr, g_.n, b.as<int32_t>());
    MSBFS_HIP_CHECK(hipGetLastError());
    deg_bounds_.assign(kDegBounds, 0);
    MSBFS_HIP_CHECK(hipMemcpy(deg_bounds_.data(), b.p, kDegBounds * sizeof(int32_t),
                              hipMemcpyDeviceToHost));
    code_key_[0] = g_.rowptr;
    code_key_[1] = g_.col;
  }
  int k = 0;
  while (k + 1 < kDegBounds && ((int64_t)1 << k) < (int64_t)min_deg) ++k;
  return deg_bounds_[k];
}

// Prefix bound H of the untiled prefix level. Pulling the ids of [a, b) costs a column entry per
// edge into the range (every active vertex scans its prefix); pushing them costs a scattered
// atomic per edge of the range's frontier vertices only. A random source is adjacent to u with
// probability ~deg(u)/n, so with S sources u is a level-1 frontier vertex with probability
// ~S deg(u)/n: the pull pays where that is >= 1/(64 W) (a push is W atomics per edge). Measured
// with tuning pfx_h: RMAT-30 / 32 groups best at H = 32768 (level 2 33.0 -> 28.7 ms), RMAT-26 /
// 16 groups at 32768-131072 (3.38 -> 3.02 ms), RMAT-22 / 64 groups near 131072, RMAT-26 / 128
// groups (2 words) at the hub bitmap's bound.
int32_t BitparSolver::pfx_bound_n(int W, int64_t nsrc) {
  if (tun_.pfx_h > 0) return std::min(tun_.pfx_h, kPfxH);
  if (nsrc <= 0) return kPfxH;
  // (>= 2^28 vertices: 1 / 32 whatever the words, the pull's column stream and the push's
  // atomics both miss the caches there; RMAT-30 / 128-group passes: H 458752 -> the ~174K
  // vertices of degree >= 2^14, 209.0 -> 203.8 ms per 256-group step; 32 groups unchanged)
  const double md = n_eff() >= ((int64_t)1 << 28)
                        ? (double)g_.n / (32.0 * (double)nsrc)
                        : (double)g_.n / (64.0 * W * (double)nsrc);  // degree where the pull pays
  if (md < 2.0) return kPfxH;
  int k = 0;
  while (k + 1 < kDegBounds && (double)((int64_t)1 << (k + 1)) <= md) ++k;  // 2^k <= md
  const int32_t h = code_bound((double)((int64_t)1 << k));  // vertices of degree >= 2^k
  return h <= 0 ? kPfxH : std::min(std::max(h, 1024), kPfxH);
}

// Everything a run would otherwise build or allocate on first use, so that no timed run pays
// for it (the CLI's computation phase, main.cu:301-400): the vertex extent, the prefix
// lengths and first-neighbour array, the degree-bound table, and the worst-case chunk
// descriptor and source-pair buffers.
void BitparSolver::prepare(hipStream_t s) {
  load_code_objects(s);
  (void)num_cus();
  const int64_t ne = n_eff();
  if (prefix_capable(plan_graph(), tun_)) {
    prefix_lens(kPfxH, s);
    if (tiles_possible()) (void)pfx_tiles(maxW_, 0, 1, s);  // (the first pull level's tiles)
  }
  if (tun_.lean) first_nbr(s);
  (void)leaf_fold_for(false, 1, false, s);  // (the parent lists of leaf folding, where it applies)
  if (tun_.dskip) dsnap_.ensure(std::max<size_t>((size_t)((g_.n + 31) / 32) * sizeof(uint32_t), 4));
  (void)code_bound(1.0);
  DevBuf c;
  c.alloc(sizeof(unsigned long long));
  MSBFS_HIP_CHECK(hipMemsetAsync(c.p, 0, sizeof(unsigned long long), s));
  k_count_wide<<<grid_for(g_.n, kBlock, 2048), kBlock, 0, s>>>(g_.rowptr, g_.n, opt.wide_degree,
                                                               c.as<unsigned long long>());
  MSBFS_HIP_CHECK(hipGetLastError());
  unsigned long long nwide = 0;
  MSBFS_HIP_CHECK(hipMemcpyAsync(&nwide, c.p, sizeof(nwide), hipMemcpyDeviceToHost, s));
  MSBFS_HIP_CHECK(hipStreamSynchronize(s));
  const size_t db = (size_t)(nwide + g_.nnz / kChunk + 1) * sizeof(ChunkDesc);
  size_t fr = 0, tot = 0;
  MSBFS_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if (db < fr / 8) desc_.ensure(db);  // (a graph filling HBM keeps the per-level sizing)
  pairs_.ensure((size_t)1 << 22);
  prof_reserve(maxW_, kProfBins);  // (a profile run of the default bin count allocates nothing)
  (void)ne;
}

// The query-dependent half of prepare(): the untiled prefix level reads the prefix lengths of the
// bound its batch's source count selects (pfx_bound), cached for one bound. Built here for the
// first untiled batch of these groups (the batches split as in run()), so that the first run of
// a few-group step does not build them (RMAT-26: ~0.9 ms, RMAT-30: ~11 ms; round-5 review).
// Tiled batches read no prefix lengths.
void BitparSolver::prepare_queries(int64_t K, const int64_t* qoff, const int32_t* qids,
                                   hipStream_t s) {
  if (K <= 0) return;
  const int mw = std::min(maxW_, opt.max_words);
  // the pinned staging of the batches' masks and source pairs (start_batch): pinning host
  // memory on the first run cost ~1.9 ms of its level 1 (RMAT-26 / 1024 groups, round 6)
  {
    int64_t np_max = 1;
    for (Batch b = batch_at(K, 0, mw); b.k0 < K; b = batch_at(K, b.k0 + b.nb, mw))
      np_max = std::max<int64_t>(np_max, qoff[b.k0 + b.nb] - qoff[b.k0]);
    const size_t hbytes = 32 * sizeof(uint64_t) + (size_t)np_max * 2 * sizeof(int32_t);
    if (!hsrc_ || hsrc_->bytes < hbytes) hsrc_ = std::make_unique<PinnedBuf>(hbytes + hbytes / 2);
    pairs_.ensure((size_t)np_max * 2 * sizeof(int32_t));
    leaf_.first.ensure((size_t)np_max);
  }
  if (!prefix_capable(plan_graph(), tun_)) {
    MSBFS_HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  for (Batch b = batch_at(K, 0, mw); b.k0 < K; b = batch_at(K, b.k0 + b.nb, mw)) {
    if (tiles_possible() && b.w >= 4 && b.w >= tun_.tiles_w) continue;  // (tiled)
    int64_t nsrc = 0;
    for (int64_t j = qoff[b.k0]; j < qoff[b.k0 + b.nb]; ++j) nsrc += qids[j] >= 0 && qids[j] < g_.n;
    prefix_lens(pfx_bound_n(b.w, nsrc), s);
    break;
  }
  MSBFS_HIP_CHECK(hipStreamSynchronize(s));
}

// dskip (see pull_full.hpp). Rows are skipped only by the lean first-row pass (and its overflow
// pull): there ~98 % of the active vertices finish (RMAT-26 level 4: 24.4M rows not written).
// Measured (round 4, RMAT-26 / 1024 groups): probing on every unfiltered level cost level 3
// +0.55 ms (a dependent 4-byte load per step for vertices whose neighbours are never done) for
// -0.25 ms at level 4. A vertex done at a skipping level L keeps a stale row, so every later pull
// level of the batch probes a snapshot of the done bitmap taken at the start of level L + 1
// (one copy: vertices done after it wrote their rows); level L itself probes the snapshot of its
// own start (its first neighbours: a done hub covers the vertex without a row gather).
const uint32_t* BitparSolver::done_probe(Loop& S, bool skip_now, hipStream_t s) {
  if (!skip_now && !S.skipped_any) return nullptr;
  const size_t b = (size_t)((g_.n + 31) / 32) * sizeof(uint32_t);
  if (skip_now || S.resnap) {
    dsnap_.ensure(std::max<size_t>(b, 4));
    MSBFS_HIP_CHECK(hipMemcpyAsync(dsnap_.p, done_.p, b, hipMemcpyDeviceToDevice, s));
  }
  S.resnap = skip_now;
  S.skipped_any |= skip_now;
  return dsnap_.as<uint32_t>();
}

// rows of the last (dskip) pull level's frontier vertices that finished there (see
// k_fix_done_rows); the level's output buffer is vis_[cur], its input vis_[cur ^ 1]
template <int W>
void BitparSolver::fix_done_rows(Loop& S, hipStream_t s) {
  S.skip_pending = false;
  if (S.nf <= 0) return;
  const Small sm = small();
  k_fix_done_rows<W><<<cap(grid_for(S.nf, Lay<W>::TILE, kMaxGrid)), kBlock, 0, s>>>(
      fl_[S.fc].as<int32_t>(), nullptr, S.nf, done_.as<uint32_t>(),
      vis_[S.cur ^ 1].as<uint64_t>(), vis_[S.cur].as<uint64_t>(), S.skip_alive, sm.gmask);
  MSBFS_HIP_CHECK(hipGetLastError());
}

PlanLevel BitparSolver::plan_level(const Loop& S) const {
  PlanLevel l;
  l.level = S.level;
  l.stop_level = S.stop_level;
  l.bu_levels = S.bu_levels;
  l.nparts = S.nparts;
  l.lazy = S.lazy;
  l.lean_off = S.lean_off;
  l.keep_rows = S.keep_rows;
  l.skipped_any = S.skipped_any;
  l.on_chunk = (bool)S.on_chunk;
  l.have_active = S.have_active;
  l.old_stale = S.old_stale;
  l.fsrc_acc = S.fsrc_acc;
  l.ev = S.ev;
  l.ef0 = S.ef0;
  l.nact = S.nact;
  l.nactw = S.nactw;
  l.na = S.na;
  return l;
}

template <int W, class Cfg>
void BitparSolver::launch_narrow(int grid, const PullArgs& a, hipStream_t s, const PullPlan* p) {
  // the plan states the launch shape (PullPlan::block / minw / hub_w), the variant has it built
  // in: they must agree
  if (p && (p->block != Cfg::BT || p->minw != Cfg::MINW || p->hub_w != Cfg::HUBW))
    fail("k_bu_narrow: the variant's launch shape is not the plan's");
  k_bu_narrow<W, Cfg><<<grid, Cfg::BT, 0, s>>>(a.list, a.nact, g_.rowptr, g_.col, a.R, a.O, a.alive, small().gmask,
                           done_.as<uint32_t>(), a.act2, a.fl2, a.ctr, anyvis_.as<uint32_t>(),
                           a.filter_from, a.actw2, std::max(opt.wide_degree, kWideLater), a.slab,
                           a.pacc, a.stamp, a.epoch, a.plen, a.nact_dev, a.snap, a.gate);
}
template <class K>
void BitparSolver::launch_full(K k, int grid, const PullArgs& a, hipStream_t s) {
  k<<<grid, kBlock, 0, s>>>(a.list, a.nact, g_.rowptr, g_.col, a.R, a.O, g_.n, a.alive,
                            small().gmask, done_.as<uint32_t>(), a.act2, a.fl2, a.ctr,
                            anyvis_.as<uint32_t>(), a.actw2, std::max(opt.wide_degree, kWideLater),
                            a.slab, a.nact_dev, a.gate, a.dprobe, a.flags);
}

// the first pull level of a batch (or the first after push levels) builds its active lists
void BitparSolver::bu_build_lists(Loop& S, BuLevel& L, hipStream_t s) {
  const PullPlan& p = L.p;
  k_build_active<4096><<<grid_for(S.cnt, 4096, INT32_MAX), kBlock, 0, s>>>(
      S.cnt, S.part, S.nparts, g_.rowptr, done_.as<uint32_t>(), p.wide0, act_[0].as<int32_t>(),
      actw_[0].as<int32_t>(), ctr_.as<Ctr>(), p.pfx_lists ? prefix_lens(L.H, s) : nullptr,
      (p.pfx_lists && g_.old2new) ? n_eff() : -1);  // (degree-relabelled: no isolated id < n_eff)
  MSBFS_HIP_CHECK(hipGetLastError());
  const HostCtr c = read_ctr(s);
  S.nact = c.act2;
  S.nactw = c.actw2;
  S.have_active = true;
  MSBFS_HIP_CHECK(hipMemsetAsync(ctr_.p, 0, sizeof(Ctr), s));
}

// the any-visited snapshot of a lazy batch's first pull and the done snapshot of dskip
void BitparSolver::bu_snapshots(Loop& S, BuLevel& L, hipStream_t s) {
  const PullPlan& p = L.p;
  if (p.lazy_first) {
    MSBFS_HIP_CHECK(hipMemcpyAsync(asnap_.p, anyvis_.p, anyvis_.bytes, hipMemcpyDeviceToDevice, s));
    L.snap = asnap_.as<uint32_t>();
  }
  if (p.take_snapshot) L.dsnap = done_probe(S, p.skip_now || p.skip3, s);
  L.dprobe = p.probe ? L.dsnap : nullptr;
  S.skip_pending = p.skip_now || p.skip3;
  S.skip_alive = L.alive;
}

// Sparse row codes (see k_build_codes). With the prefix pull only ids < H and the tail pushers'
// own codes are ever read: the codes of [code_from, H) plus those of the frontier vertices >= H
// (not 4 bytes for every id).
template <int W>
void BitparSolver::bu_codes(Loop& S, BuLevel& L, hipStream_t s) {
  const PullPlan& p = L.p;
  L.code_from = kNoCodes;
  if (!p.codes) return;
  const int64_t ne = n_eff();
  const int32_t from = (int32_t)std::min<int64_t>(
      code_bound(p.code_deg * (double)g_.nnz / (double)S.ef0), ne);
  if (from >= ne) return;
  uint32_t* cb = touched_.as<uint32_t>();  // n entries
  const int64_t hi = p.pfx ? std::min<int64_t>(std::max<int64_t>(kPfxH, from), ne) : ne;
  const int64_t nl = p.pfx ? S.nf : 0;
  k_build_codes<W><<<grid_for(hi - from + nl, kBlock, 8192), kBlock, 0, s>>>(
      L.R, anyvis_.as<uint32_t>(), from, hi, fl_[S.fc].as<int32_t>(), nl, cb);
  MSBFS_HIP_CHECK(hipGetLastError());
  L.codes = cb;
  L.code_from = from;
}

// The prefix level's set-up: prefix lengths of the per-vertex pull (plen is cached for one bound:
// a batch with another source count rebuilds it, one pass over the rows; the tiles hold their
// entries: no prefix lengths read at run time), the frontier bitmap, and the tail push before
// the pulls (see k_push_tail).
template <int W>
void BitparSolver::bu_tail_push(Loop& S, BuLevel& L, hipStream_t s) {
  const PullPlan& p = L.p;
  L.plen = p.pfx && !p.tiled ? prefix_lens(L.H, s) : nullptr;
  if (p.fbm_out) {
    const int64_t nwords = (g_.n + 31) / 32;
    fbm_tile_.ensure((size_t)(nwords + 1) * sizeof(uint32_t));
    MSBFS_HIP_CHECK(hipMemsetAsync(fbm_tile_.p, 0, (size_t)nwords * sizeof(uint32_t), s));
  }
  S.push_after = p.push_after;
  if (!p.tail_push) return;
  ++epoch_;
  const int split = S.nf < 65536 ? 8 : 1;  // (see k_push_tail)
  k_push_tail<W><<<cap(grid_for(S.nf * 64 * split, kBlock, 8192)), kBlock, 0, s>>>(
      fl_[S.fc].as<int32_t>(), S.nf, L.H, g_.rowptr, g_.col, L.R, L.codes, L.code_from,
      p.tiled ? nullptr : done_.as<uint32_t>(), S.part, S.nparts, acc_[S.ac].as<uint64_t>(),
      (p.tiled || p.pfx_nostamp) ? nullptr : stamp_.as<int32_t>(), epoch_, split, push_bound(S));
  MSBFS_HIP_CHECK(hipGetLastError());
}

// the narrow-list pull, by the plan's kind
template <int W, bool COUNT>
void BitparSolver::bu_narrow(Loop& S, BuLevel& L, hipStream_t s) {
  using Lw = Lay<W>;
  // (the edge-counting pass counts with k_count_frontier: nothing fused there)
  constexpr bool FUSE = !COUNT;
  const PullPlan& p = L.p;
  if (p.kind == PullKind::Tiled) {
    L.rows = tiles_pull<W>(S, s, L.R, L.O, L.snap, L.codes, L.code_from, L.rows);
    if (S.push_after) {
      const int gp = cap(grid_for(S.nf * 64, kBlock, kMaxGrid));
      if (L.rows + gp > 3 * kMaxGrid) fail("tail push: counter slab rows exhausted");
      k_push_tail_after<W><<<gp, kBlock, 0, s>>>(
          fl_[S.fc].as<int32_t>(), S.nf, kPfxH, g_.rowptr, g_.col, L.R, L.codes, L.code_from, L.O,
          fbm_tile_.as<uint32_t>(), anyvis_.as<uint32_t>(), ctr_.as<Ctr>(), slabF<W>(L.rows),
          push_bound(S));
      MSBFS_HIP_CHECK(hipGetLastError());
      L.rows += gp;
      S.push_after = false;
    }
    S.have_active = S.level < S.stop_level;
    return;
  }
  if (!S.nact) return;
  PullArgs a{act_[0].as<int32_t>(), S.nact, L.R, L.O, L.alive, act_[1].as<int32_t>(),
             actw_[1].as<int32_t>(), fl_[S.fc ^ 1].as<int32_t>(), ctr_.as<Ctr>(),
             slabF<W>(L.rows)};
  a.filter_from = p.filter_from;
  a.snap = L.snap;
  const int gn = cap(grid_for(S.nact, Lw::TILE, kMaxGrid));  // (the 256-thread kernels)
  switch (p.kind) {
    case PullKind::Prefix: {
      using Cfg = NarrowPrefix<W, FUSE>;
      const int g = cap(grid_for(S.nact, (Cfg::BT / 64) * Lw::VPW, 512));
      if (Cfg::FBM) a.fl2 = reinterpret_cast<int32_t*>(fbm_tile_.p);
      a.pacc = acc_[S.ac].as<uint64_t>();
      a.stamp = p.pfx_nostamp ? nullptr : stamp_.as<int32_t>();
      a.epoch = epoch_;
      a.plen = L.plen;
      launch_narrow<W, Cfg>(g, a, s, &p);
      if (FUSE) L.rows += g;
      break;
    }
    case PullKind::Hub: {
      const int g = cap(grid_for(S.nact, (NarrowHub<FUSE>::BT / 64) * Lw::VPW, 512));
      if (p.hub_big) launch_narrow<W, NarrowHubBig<FUSE>>(g, a, s, &p);
      else launch_narrow<W, NarrowHub<FUSE>>(g, a, s, &p);
      if (FUSE) L.rows += g;
      break;
    }
    case PullKind::Lean: {
      // lean first pass, then the regular pull over the vertices it could not finish
      S.lean_ran = true;
      k_bu_first<W><<<gn, kBlock, 0, s>>>(
          a.list, S.nact, g_.rowptr, g_.col, L.R, L.O, L.alive, L.sm.gmask, done_.as<uint32_t>(),
          touched_.as<int32_t>(), a.fl2, a.ctr, anyvis_.as<uint32_t>(), slabF<W>(L.rows),
          first_nbr(s), L.dsnap, p.skip_now ? kFlagSkipRows : 0);
      MSBFS_HIP_CHECK(hipGetLastError());
      L.rows += gn;
      const int go = p.full ? full_grid<W>(gn, S.nact, true) : gn;
      a.list = touched_.as<int32_t>();
      a.slab = slabF<W>(L.rows);
      a.nact_dev = &ctr_.as<Ctr>()->touched.v;
      a.dprobe = L.dsnap;
      a.flags = p.skip_now ? kFlagSkipRows : 0;
      if (p.full) launch_full(k_bu_full<W, full_cs<W>(), 1>, go, a, s);
      else if constexpr (FUSE) launch_narrow<W, NarrowShort1<true>>(go, a, s, &p);
      else fail("the lean pass is not planned for an edge-counting run");
      L.rows += go;
      break;
    }
    case PullKind::Full: {
      const int gf = full_grid<W>(gn, S.nact);
      a.dprobe = L.dprobe;
      a.flags = p.skip3 ? kFlagSkipRows : 0;
      launch_full(p.short1 ? k_bu_full<W, full_cs<W>(), 1> : k_bu_full<W, full_cs<W>(), 0>, gf, a, s);
      L.rows += gf;
      break;
    }
    default: {
      // (the short first step only where the counts are fused: no NarrowShort1<false> exists)
      bool short1 = false;
      if constexpr (FUSE) {
        short1 = !p.filter && p.short1;
        if (short1) launch_narrow<W, NarrowShort1<true>>(gn, a, s, &p);
      }
      if (p.filter) launch_narrow<W, NarrowFiltered<FUSE>>(gn, a, s, &p);
      else if (!short1) launch_narrow<W, NarrowPlain<FUSE>>(gn, a, s, &p);
      if (FUSE) L.rows += gn;
    }
  }
  MSBFS_HIP_CHECK(hipGetLastError());
}

// one launch over chunk descriptors d[0 .. *np) (exact count read on the device: no host round
// trip), at most maxc of them
template <int W>
void BitparSolver::bu_chunks(Loop& S, BuLevel& L, const ChunkDesc* d, const int64_t* np,
                             int64_t maxc, hipStream_t s) {
  const PullPlan& p = L.p;
  auto ck = !p.hub_lds                   ? k_bu_chunks<W, 256, kBlock, 0>
            : p.chunk_hub_big            ? k_bu_chunks<W, 256, 1024, kHubBig>
            : (p.chunk_pfxl && !L.codes) ? k_bu_chunks<W, 256, 1024, kHubW, true>
                                         : k_bu_chunks<W, 256, 1024, kHubW>;
  const int grid = !p.hub_lds ? grid_for(maxc, kWaves, 8192)
                              : grid_for(maxc, 16, p.chunk_hub_big ? 256 : 512);
  ck<<<grid, p.hub_lds ? 1024 : kBlock, 0, s>>>(
      d, np, g_.col, L.R, L.alive, L.sm.gmask, acc_[S.ac].as<uint64_t>(), anyvis_.as<uint32_t>(),
      p.filter_from, p.coop, L.codes, L.code_from, L.snap, L.dprobe);
  MSBFS_HIP_CHECK(hipGetLastError());
}

// the wide vertices: chunk descriptors (by the plan's scheduling), chunk launches, finalize
template <int W, bool COUNT>
void BitparSolver::bu_wide(Loop& S, BuLevel& L, hipStream_t s) {
  using Lw = Lay<W>;
  constexpr bool FUSE = !COUNT;
  const PullPlan& p = L.p;
  if (!S.nactw || p.tiled) return;
  const int32_t* lw = actw_[0].as<int32_t>();
  const int64_t chunks_max = S.nactw + S.ea / kChunk + 1;
  desc_.ensure((size_t)chunks_max * sizeof(ChunkDesc));
  ChunkDesc* d = desc_.as<ChunkDesc>();
  // (scan scratch behind the per-vertex counts)
  int64_t* cnt = scan_tmp_.as<int64_t>();
  char* t2 = (char*)scan_tmp_.p + (((size_t)S.nactw * sizeof(int64_t) + 255) & ~size_t(255));
  const size_t tb = scan_bytes_ - (size_t)(t2 - (char*)scan_tmp_.p);
  if (p.chunks == ChunkSched::TwoPass) {
    chunk_cnt_.ensure(sizeof(int64_t));
    k_chunk_first<<<grid_for(S.nactw, kBlock), kBlock, 0, s>>>(lw, S.nactw, g_.rowptr, d,
                                                                chunk_cnt_.as<int64_t>());
    MSBFS_HIP_CHECK(hipGetLastError());
    bu_chunks<W>(S, L, d, chunk_cnt_.as<int64_t>(), S.nactw, s);
    k_chunk_rest_count<W><<<cap(grid_for(S.nactw, Lw::TILE, kMaxGrid)), kBlock, 0, s>>>(
        lw, S.nactw, g_.rowptr, L.R, acc_[S.ac].as<uint64_t>(), L.alive, L.sm.gmask, L.snap, cnt);
    MSBFS_HIP_CHECK(hipGetLastError());
    inclusive_scan_i64(cnt, offs_.as<int64_t>(), S.nactw, t2, tb, s);
    k_chunk_rest_desc<<<grid_for(S.nactw, kBlock), kBlock, 0, s>>>(
        lw, S.nactw, offs_.as<int64_t>(), g_.rowptr, d + S.nactw);
    MSBFS_HIP_CHECK(hipGetLastError());
    bu_chunks<W>(S, L, d + S.nactw, offs_.as<int64_t>() + S.nactw - 1, chunks_max - S.nactw, s);
  } else {
    if (p.chunks == ChunkSched::Prefix) {
      k_prefix_chunks<<<grid_for(S.nactw, kBlock), kBlock, 0, s>>>(lw, S.nactw, L.plen, cnt);
      MSBFS_HIP_CHECK(hipGetLastError());
      inclusive_scan_i64(cnt, offs_.as<int64_t>(), S.nactw, t2, tb, s);
    } else {
      frontier_degree_scan(g_.rowptr, lw, S.nactw, offs_.as<int64_t>(), scan_tmp_.p, scan_bytes_,
                           s, kChunk);
    }
    k_chunk_desc<<<grid_for(S.nactw, kBlock), kBlock, 0, s>>>(lw, S.nactw, offs_.as<int64_t>(),
                                                               g_.rowptr, L.plen, d);
    MSBFS_HIP_CHECK(hipGetLastError());
    bu_chunks<W>(S, L, d, offs_.as<int64_t>() + S.nactw - 1, chunks_max, s);
  }
  const int gw = cap(grid_for(S.nactw, Lw::TILE, kMaxGrid));
  auto kw = p.fbm_out ? k_bu_wide_finalize<W, FUSE, true> : k_bu_wide_finalize<W, FUSE>;
  kw<<<gw, kBlock, 0, s>>>(
      lw, S.nactw, g_.rowptr, L.R, L.O, acc_[S.ac].as<uint64_t>(), L.alive, L.sm.gmask,
      done_.as<uint32_t>(), actw_[1].as<int32_t>(), fl_[S.fc ^ 1].as<int32_t>(), ctr_.as<Ctr>(),
      anyvis_.as<uint32_t>(), act_[1].as<int32_t>(), p.next_wide, slabF<W>(L.rows), L.snap,
      p.fbm_out ? fbm_tile_.as<uint32_t>() : nullptr);
  MSBFS_HIP_CHECK(hipGetLastError());
  if (FUSE) L.rows += gw;
}

// One bottom-up level: the plan (bitpar/pull_plan.hpp), then its stages in order.
template <int W, bool COUNT>
int BitparSolver::level_bu(Loop& S, hipStream_t s) {
  BuLevel L;
  L.sm = small();
  L.R = vis_[S.cur].as<uint64_t>();
  L.O = vis_[S.cur ^ 1].as<uint64_t>();
  L.alive = L.sm.alive[S.alv];
  if (S.old_stale) {
    // fused top-down levels wrote only vis_[cur]; pulls write the other buffer's rows of the
    // active vertices and read both buffers' rows of the finished ones afterwards
    const size_t vb = (size_t)std::max<int64_t>(n_eff(), 1) * W * sizeof(uint64_t);
    MSBFS_HIP_CHECK(hipMemcpyAsync(L.O, L.R, vb, hipMemcpyDeviceToDevice, s));
    S.old_stale = false;
  }
  const PlanGraph g = plan_graph();
  const PlanOpts o{opt.wide_degree, kDefaultWideDegree};
  PlanLevel l = plan_level(S);
  // (asking for the tiles builds them on first use: only once the level wants them)
  const bool tiled =
      wants_tiles(g, tun_, W, COUNT, l) && pfx_tiles(W, S.part, S.nparts, s) != nullptr;
  l.H = L.H = tiled ? kPfxH : pfx_bound<W>(S);
  S.fl_bitmap = false;  // this level writes its own frontier (list, or bitmap when tiled)
  plan_lists(L.p, g, o, tun_, W, l, tiled);
  if (L.p.build_lists) bu_build_lists(S, L, s);
  l.nact = S.nact;
  l.nactw = S.nactw;
  L.p = plan_pull(g, o, tun_, W, COUNT, l, tiled);
  const PullPlan& p = L.p;
  ++S.bu_levels;
  S.kind = (char)p.kind;
  if (S.fsrc_acc) {
    // bottom-up does not read frontier bits; clear the pending top-down ones so acc_[ac]
    // is all-zero and can collect the wide vertices' chunk results
    k_zero_acc<W><<<cap(grid_for(S.nf * Lay<W>::G, kBlock)), kBlock, 0, s>>>(
        fl_[S.fc].as<int32_t>(), S.nf, acc_[S.ac].as<uint64_t>());
    MSBFS_HIP_CHECK(hipGetLastError());
  }
  bu_snapshots(S, L, s);
  bu_codes<W>(S, L, s);
  bu_tail_push<W>(S, L, s);
  bu_narrow<W, COUNT>(S, L, s);
  bu_wide<W, COUNT>(S, L, s);
  if constexpr (COUNT) {
    // the edge-counting mode's count pass (the traversal kernels fuse the plain counts):
    // new frontier bits = Wb & ~R (both still in place: the swap is below)
    const int gc = cap(grid_for(S.nact + S.nactw, Lay<W>::TILE, kMaxGrid));
    k_count_frontier<W, COUNT, true><<<gc, kBlock, 0, s>>>(
        fl_[S.fc ^ 1].as<int32_t>(), ctr_.as<Ctr>(), g_.rowptr, L.O, L.R, slabF<W>(L.rows),
        slabE<W>(L.rows));
    MSBFS_HIP_CHECK(hipGetLastError());
    L.rows += gc;
    record_level<W, true>(fl_[S.fc ^ 1].as<int32_t>(), ctr_.as<Ctr>(), L.O, L.R,
                          S.nact + S.nactw, cap(kMaxGrid), S.level, s);
  }
  std::swap(act_[0], act_[1]);
  std::swap(actw_[0], actw_[1]);
  S.cur ^= 1;
  S.fsrc_acc = false;
  S.osnap_next = p.lazy_first;
  if (p.fbm_out) S.fl_bitmap = true;
  return L.rows;
}

// A batch of up to bu_next_ pull levels with no host synchronisation (the late levels of
// scale-free graphs: RMAT levels 4+ cost ~10-50 us of GPU time each, less than a host round
// trip). Level i reads counter slot i (slot 0 seeded from the host) and writes slot i + 1; its
// kernels run only while the BuGate on slot i is open (frontier non-empty and the pull -> push
// test still says pull), so the levels after the frontier dies or the direction turns are
// no-ops and the host loop resumes exactly where the host-driven levels would be. Both lists
// (narrow, wide) go through the short-first-step narrow kernel (late levels: most vertices are
// covered by their first neighbour); the list lengths come from the slots.
template <int W, bool COUNT>
void BitparSolver::bu_batch(Loop& S, RunStats* st, hipStream_t s) {
  static_assert(!COUNT, "edge counting keeps host-driven pull levels (bu_batch_ok)");
  using L = Lay<W>;
  const Small sm = small();
  int K = std::max(2, std::min({bu_next_, tun_.batch, kBatch}));
  if (S.stop_level != 0xFFFFFFFFu) K = (int)std::min<int64_t>(K, (int64_t)S.stop_level - S.level);
  S.fl_bitmap = false;  // (the batch's levels write frontier lists)
  Ctr* slots = bctr_.as<Ctr>();
  uint64_t* aslot = (uint64_t*)(slots + kBatch + 1);
  MSBFS_HIP_CHECK(hipMemsetAsync(bctr_.p, 0, bctr_.bytes, s));
  k_bu_seed<<<1, 64, 0, s>>>(slots, (uint32_t)S.nf, (unsigned long long)S.ef, (uint32_t)S.nact,
                             (uint32_t)S.nactw, (unsigned long long)S.ea, sm.alive[S.alv], aslot);
  MSBFS_HIP_CHECK(hipGetLastError());
  // lists only shrink: a vertex stays active at most, and keeps its side of the kWideLater split
  const int g0 = cap(grid_for(S.nact + S.nactw, L::TILE, kMaxGrid));
  const int gn = full_pull() ? full_grid<W>(g0, S.nact, true) : g0;
  const int gw = S.nactw ? cap(grid_for(S.nactw, L::TILE, kMaxGrid)) : 0;
  const int rows = gn + gw, rg = std::max(1, std::min(64, rows / 32));
  const double alpha = alpha_eff();
  const uint32_t level0 = S.level;
  const auto t0 = std::chrono::steady_clock::now();
  trace::Range range_batch("bitpar L%u-%u BU batch", level0 + 1, level0 + K);
  const bool full = full_pull();
  // dskip: after a skipping level the batch's levels probe the snapshot (taken once, before the
  // first of them); they skip nothing themselves
  const uint32_t* dsnap = full ? done_probe(S, false, s) : nullptr;
  auto launch = [&](int grid, const int32_t* list, const uint64_t* R, uint64_t* O,
                    const uint64_t* alive, int32_t* fl_out, Ctr* out, uint32_t* slab,
                    const uint32_t* len, const BuGate& gate, int p) {
    PullArgs a{list, 0, R, O, alive, act_[p ^ 1].as<int32_t>(), actw_[p ^ 1].as<int32_t>(),
               fl_out, out, slab};
    a.nact_dev = len;
    a.gate = gate;
    a.dprobe = dsnap;
    if (full) launch_full(k_bu_full<W, full_cs<W>(), 1>, grid, a, s);
    else launch_narrow<W, NarrowShort1<true>>(grid, a, s);
  };
  for (int i = 0; i < K; ++i) {
    const BuGate gate{slots + i, opt.beta, alpha, i == 0 ? 1 : 0};
    const int p = i & 1;
    const uint64_t* R = vis_[S.cur ^ p].as<uint64_t>();
    uint64_t* O = vis_[S.cur ^ p ^ 1].as<uint64_t>();
    int32_t* fl_out = fl_[S.fc ^ p ^ 1].as<int32_t>();
    const uint64_t* alive = aslot + 16 * i;
    launch(gn, act_[p].as<int32_t>(), R, O, alive, fl_out, slots + i + 1, slabF<W>(0),
           &slots[i].act2.v, gate, p);
    if (gw)
      launch(gw, actw_[p].as<int32_t>(), R, O, alive, fl_out, slots + i + 1, slabF<W>(gn),
             &slots[i].actw2.v, gate, p);
    k_level_reduce<W, false><<<W * rg, kBlock, 0, s>>>(slabF<W>(0), slabE<W>(0), rows, rg, sm.F,
                                                       sm.E, aslot + 16 * (i + 1), level0 + 1 + i,
                                                       gate, prof_at(level0 + 1 + i));
    MSBFS_HIP_CHECK(hipGetLastError());
    // (a closed level appends nothing: its list is empty)
    if (S.fold) leaf_weigh<W>(O, alive, level0 + 2 + i, fl_out, 0, &slots[i + 1].fl2.v, s);
  }
  MSBFS_HIP_CHECK(hipMemcpyAsync(hbctr_->p, bctr_.p, (size_t)(K + 1) * sizeof(Ctr),
                                 hipMemcpyDeviceToHost, s));
  MSBFS_HIP_CHECK(hipStreamSynchronize(s));
  const Ctr* h = hbctr_->as<Ctr>();
  int real = 0;  // levels whose gate was open (the same test the kernels made)
  while (real < K && bu_gate_eval(h[real], opt.beta, alpha, real == 0 ? 1 : 0)) {
    S.ev += (int64_t)h[real + 1].ev2.v;
    ++real;
  }
  MSBFS_HIP_CHECK(hipMemcpyAsync(sm.alive[S.alv], aslot + 16 * real, 16 * sizeof(uint64_t),
                                 hipMemcpyDeviceToDevice, s));
  if (st && real > 0) {  // per-level records; the batch's wall time is split evenly
    const double ms = std::chrono::duration<double, std::milli>(
                          std::chrono::steady_clock::now() - t0).count() / real;
    for (int i = 0; i < real; ++i) {
      LevelRec rec;
      rec.batch = (int32_t)st->batches;
      rec.level = (int32_t)(level0 + 1 + i);
      rec.dir = 'B';
      rec.kind = (char)batch_kind(plan_graph());
      rec.nf = h[i].fl2.v;
      rec.ef = (int64_t)h[i].ef2.v;
      rec.nf_next = h[i + 1].fl2.v;
      rec.active = (int64_t)h[i + 1].act2.v + h[i + 1].actw2.v;  // (as levels(): the new lists)
      rec.ms = ms;
      st->recs.push_back(rec);
    }
    st->bu_levels += real;
    st->levels += real;
  }
  S.level = level0 + real;
  S.bu_levels += real;
  S.nf = h[real].fl2.v;
  S.ef = (int64_t)h[real].ef2.v;
  S.nact = h[real].act2.v;
  S.nactw = h[real].actw2.v;
  S.na = S.nact + S.nactw;
  S.ea = (int64_t)h[real].eu2.v;
  if (real & 1) {  // level i read list / row / frontier buffers of parity i
    std::swap(act_[0], act_[1]);
    std::swap(actw_[0], actw_[1]);
    S.cur ^= 1;
    S.fc ^= 1;
  }
  S.fsrc_acc = false;
  S.osnap_next = false;
  // (the last real level's alive mask stays in bctr_ until the next batch: a push level right
  // after restores the skipped rows of its frontier first, see levels())
  if (real > 0) S.skip_pending = false;  // (a skipping level's frontier: restored only if next)
  // the next batch: twice as long while the frontier lives, else this tail's length + 1
  bu_next_ = real == K ? std::min(2 * K, kBatch) : real + 1;
}


// ---- leaf folding (bitpar/leaf.hpp) -------------------------------------------------------------
int64_t BitparSolver::leaf_n_core() {
  if (leaf_.key[0] != (const void*)g_.rowptr || leaf_.key[1] != (const void*)g_.col ||
      leaf_.key[2] != (const void*)g_.old2new) {
    leaf_ = LeafState{};
    leaf_.key[0] = g_.rowptr;
    leaf_.key[1] = g_.col;
    leaf_.key[2] = g_.old2new;
  }
  if (!leaf_.bounds) {
    const int64_t ne = n_eff();
    // (the first id of degree < 2; the table is empty for ids that are not in degree order)
    leaf_.n_core = (g_.old2new && g_.rows_sorted && g_.n <= INT32_MAX)
                       ? std::min<int64_t>(code_bound(2.0), ne)
                       : ne;
    leaf_.bounds = true;
  }
  return leaf_.n_core;
}

bool BitparSolver::leaf_fold_for(bool count, int nparts, bool limited, hipStream_t s) {
  if (tun_.leaf == 0) return false;
  LeafRun r;
  r.leaf_key = tun_.leaf;
  r.relabelled = g_.old2new != nullptr;
  r.rows_sorted = g_.rows_sorted;
  r.count = count;
  r.nparts = nparts;
  r.limited = limited;
  if (!r.relabelled || !r.rows_sorted) return false;
  if (!leaf_fold_on(r, leaf_n_core(), n_eff())) return false;
  if (!leaf_.lists && !leaf_.no_room) leaf_build(s);
  return leaf_.lists;
}

// the parents' weights (device), their lists (host, bitpar/leaf.hpp) and the count's own record
void BitparSolver::leaf_build(hipStream_t s) {
  const int64_t nc = leaf_n_core(), ne = n_eff();
  DevBuf lw((size_t)std::max<int64_t>(nc, 1) * sizeof(int32_t));
  std::vector<int32_t> hw((size_t)std::max<int64_t>(nc, 1), 0);
  if (nc > 0) {
    k_leaf_weights<<<grid_for(nc, kBlock, 8192), kBlock, 0, s>>>(g_.rowptr, g_.col, nc,
                                                                  lw.as<int32_t>());
    MSBFS_HIP_CHECK(hipGetLastError());
    MSBFS_HIP_CHECK(hipMemcpyAsync(hw.data(), lw.p, (size_t)nc * sizeof(int32_t),
                                   hipMemcpyDeviceToHost, s));
  }
  MSBFS_HIP_CHECK(hipStreamSynchronize(s));
  const LeafLists L = build_leaf_lists(hw.data(), nc, ne);
  const size_t np = (size_t)std::max<int64_t>(L.positions(), 1);
  const size_t need = np * (8 + (size_t)maxW_ * sizeof(uint64_t)) + L.pidx.size() * 4;
  size_t fr = 0, tot = 0;
  MSBFS_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if (need + ((size_t)2 << 30) > fr && need > ((size_t)64 << 20)) {  // (no room: unfolded)
    leaf_.no_room = true;
    return;
  }
  leaf_.plist.alloc(np * sizeof(int32_t));
  leaf_.pw.alloc(np * sizeof(int32_t));
  leaf_.pidx.alloc(L.pidx.size() * sizeof(int32_t));
  leaf_.seen.alloc(np * (size_t)maxW_ * sizeof(uint64_t));
  leaf_.epoch.alloc(np * sizeof(int32_t));
  leaf_.first.ensure((size_t)1 << 16);
  MSBFS_HIP_CHECK(hipMemcpyAsync(leaf_.plist.p, L.plist.data(), np * sizeof(int32_t),
                                 hipMemcpyHostToDevice, s));
  MSBFS_HIP_CHECK(hipMemcpyAsync(leaf_.pw.p, L.pw.data(), np * sizeof(int32_t),
                                 hipMemcpyHostToDevice, s));
  MSBFS_HIP_CHECK(hipMemcpyAsync(leaf_.pidx.p, L.pidx.data(), L.pidx.size() * sizeof(int32_t),
                                 hipMemcpyHostToDevice, s));
  MSBFS_HIP_CHECK(hipMemsetAsync(leaf_.epoch.p, 0, np * sizeof(int32_t), s));
  MSBFS_HIP_CHECK(hipStreamSynchronize(s));  // (L is a host object)
  leaf_epoch_ = 0;
  leaf_.parents = L.parents;
  leaf_.attached = L.attached;
  leaf_.max_w = L.max_w;
  leaf_.nsmall = L.nsmall;
  leaf_.nheavy = L.nheavy;
  leaf_.rows_dirty = true;
  leaf_.lists = true;
  if (getenv("MSBFS_TRACE"))
    fprintf(stderr,
            "[msbfs bp] leaf folding: n_core=%lld n_eff=%lld leaves=%lld (attached %lld) "
            "parents=%lld (heavy %lld) max leafw=%lld\n",
            (long long)nc, (long long)ne, (long long)(ne - nc), (long long)L.attached,
            (long long)L.parents, (long long)L.nheavy, (long long)L.max_w);
}

template <int W>
void BitparSolver::leaf_begin(Loop& S, hipStream_t s) {
  (void)S;
  if (++leaf_epoch_ == INT32_MAX) {  // (epoch 0 = never written)
    MSBFS_HIP_CHECK(hipMemsetAsync(leaf_.epoch.p, 0, leaf_.epoch.bytes, s));
    leaf_epoch_ = 1;
  }
  if (leaf_.rows_dirty || leaf_.rows_w != W) {
    const size_t off = (size_t)leaf_.n_core * W * sizeof(uint64_t);
    const size_t len = (size_t)(n_eff() - leaf_.n_core) * W * sizeof(uint64_t);
    for (int i = 0; i < 2; ++i)
      MSBFS_HIP_CHECK(hipMemsetAsync((char*)vis_[i].p + off, 0, len, s));
  }
  leaf_.rows_dirty = true;  // (until leaf_end has cleared this batch's source rows)
  leaf_.rows_w = W;
}

template <int W>
void BitparSolver::leaf_end(const int32_t* pv, int64_t np, hipStream_t s) {
  if (np > 0) {
    k_zero_src_rows<W><<<cap(grid_for(np * W, kBlock)), kBlock, 0, s>>>(
        pv, np, g_.old2new, vis_[0].as<uint64_t>(), vis_[1].as<uint64_t>());
    MSBFS_HIP_CHECK(hipGetLastError());
  }
  leaf_.rows_dirty = false;
}

template <int W>
void BitparSolver::leaf_sources(const int32_t* pv, const int32_t* pk, int64_t np, hipStream_t s) {
  const Small sm = small();
  k_leaf_sources<W><<<cap(grid_for(np, kBlock)), kBlock, 0, s>>>(
      pv, pk, leaf_.first.as<uint8_t>(), np, g_.old2new, g_.rowptr, g_.col,
      vis_[0].as<uint64_t>(), anyvis_.as<uint32_t>(), (int32_t)leaf_.n_core, (int32_t)n_eff(),
      sm.F, prof_);
  MSBFS_HIP_CHECK(hipGetLastError());
  // level 0: the parents among the sources (the first frontier list; its length is ctr's fl2)
  leaf_weigh<W>(vis_[0].as<uint64_t>(), sm.alive[0], 1, fl_[0].as<int32_t>(), 0,
                &ctr_.as<Ctr>()->fl2.v, s);
}

template <int W>
void BitparSolver::leaf_weigh(const uint64_t* R, const uint64_t* alive, uint32_t weight,
                              const int32_t* list, int64_t n, const uint32_t* n_dev,
                              hipStream_t s) {
  using L = Lay<W>;
  const Small sm = small();
  const LeafArgs a{leaf_.plist.as<int32_t>(), leaf_.pw.as<int32_t>(), leaf_.pidx.as<int32_t>(),
                   leaf_.seen.as<uint64_t>(), leaf_.epoch.as<int32_t>(), leaf_epoch_, R,
                   anyvis_.as<uint32_t>(), done_.as<uint32_t>(), alive, sm.gmask, sm.F, weight,
                   prof_};
  if (list) {
    // (a device-side length: these are the short lists of the late levels and the batches)
    const int g = cap(n_dev ? 64 : grid_for(n, kLeafU * L::TILE, 1024));
    if (!n_dev && n <= 0) return;
    k_leaf_weigh_list<W><<<g, kBlock, 0, s>>>(a, list, n, n_dev, 0, (int32_t)leaf_.n_core);
  } else {
    if (leaf_.nsmall > 0)
      k_leaf_weigh<W><<<cap(grid_for(leaf_.nsmall, kLeafU * L::TILE, 8 * std::max(1, num_cus()))),
                        kBlock, 0, s>>>(a, leaf_.nsmall);
    if (leaf_.nheavy > 0)
      k_leaf_weigh_list<W><<<cap(grid_for(leaf_.nheavy, kLeafU * L::TILE, 1024)), kBlock, 0, s>>>(
          a, nullptr, leaf_.nheavy, nullptr, leaf_.nsmall, (int32_t)leaf_.n_core);
  }
  MSBFS_HIP_CHECK(hipGetLastError());
}

#define MSBFS_BP_INST(WW)                                                 \
  template void BitparSolver::leaf_begin<WW>(Loop&, hipStream_t);        \
  template void BitparSolver::leaf_end<WW>(const int32_t*, int64_t, hipStream_t);                 \
  template void BitparSolver::leaf_sources<WW>(const int32_t*, const int32_t*, int64_t,           \
                                               hipStream_t);                                      \
  template void BitparSolver::leaf_weigh<WW>(const uint64_t*, const uint64_t*, uint32_t,          \
                                             const int32_t*, int64_t, const uint32_t*,            \
                                             hipStream_t);                                        \
  template void BitparSolver::fix_done_rows<WW>(Loop&, hipStream_t);     \
  template int BitparSolver::level_bu<WW, false>(Loop&, hipStream_t);    \
  template int BitparSolver::level_bu<WW, true>(Loop&, hipStream_t);     \
  template void BitparSolver::bu_batch<WW, false>(Loop&, RunStats*, hipStream_t);
MSBFS_BP_FOR_W(MSBFS_BP_INST)
#undef MSBFS_BP_INST

// first launch of any kernel of this translation unit loads its code object (see
// load_code_objects in bitpar/solver.hpp)
static __global__ void k_load_pull() {}
void load_code_pull(hipStream_t s) {
  k_load_pull<<<1, 64, 0, s>>>();
  MSBFS_HIP_CHECK(hipGetLastError());
}

}  // namespace bp
}  // namespace msbfs
