// Bit-parallel MS-BFS solver: construction, tuning, batches and the level loop (direction
// choice, per-level reductions, host read-back). The level bodies live in bitpar_push.hip
// (top-down) and bitpar_pull.hip (bottom-up); design overview in bitpar/solver.hpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bitpar/init.hpp"
#include "bitpar/solver.hpp"

namespace msbfs {
namespace bp {

// ---- construction ----------------------------------------------------------------------------
BitparSolver::BitparSolver(const DeviceGraph& g, int max_groups)
    : g_(g), tun_(Tuning::process_default()) {
  int w = 1;
  while (w * 64 < max_groups && w < 16) w <<= 1;
  const int64_t n = std::max<int64_t>(g.n, 1);
  // Size the batch width to free HBM: 4 visited/accumulator buffers of n*W words plus ~48 B
  // per vertex of lists; groups beyond 64*W run as further batches.
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
      const double fixed = 52.0 * (double)n + (double)g.nnz / 256.0 + 64.0 * (1 << 20);
      while (w > 1 && fixed + 32.0 * (double)n * w > 0.92 * (double)free_b) w >>= 1;
      if (fixed + 32.0 * (double)n * w > 0.92 * (double)free_b)
        fail("not enough device memory for the bit-parallel solver (n=" + std::to_string(n) + ")");
    }
  }
  maxW_ = w;
  // (+ 2 rows: the all-zero row n and the scratch row n + 1 of k_bu_full's branch-free gathers)
  const size_t vb = (size_t)(n + 2) * maxW_ * sizeof(uint64_t);
  for (int i = 0; i < 2; ++i) {
    vis_[i].alloc(vb);
    acc_[i].alloc(vb);
    MSBFS_HIP_CHECK(hipMemset(acc_[i].p, 0, vb));
  }
  stamp_.alloc((size_t)n * sizeof(int32_t));
  MSBFS_HIP_CHECK(hipMemset(stamp_.p, 0xFF, stamp_.bytes));
  done_.alloc((size_t)((n + 31) / 32) * sizeof(uint32_t));
  anyvis_.alloc((size_t)((n + 31) / 32) * sizeof(uint32_t));
  asnap_.alloc((size_t)((n + 31) / 32) * sizeof(uint32_t));
  for (int i = 0; i < 2; ++i) {
    act_[i].alloc((size_t)n * sizeof(int32_t));
    actw_[i].alloc((size_t)n * sizeof(int32_t));
    fl_[i].alloc((size_t)n * sizeof(int32_t));
  }
  touched_.alloc((size_t)n * sizeof(int32_t));
  offs_.alloc((size_t)n * sizeof(int64_t));
  scan_bytes_ = frontier_scan_temp_bytes(n);
  scan_tmp_.alloc(scan_bytes_);
  ctr_.alloc(sizeof(Ctr));
  // F, E, alive x 2, gmask, (spare) (see Small)
  small_.alloc(64 * 16 * sizeof(unsigned long long) * 3 + 4 * 16 * sizeof(uint64_t));
  // per-level counter slab: <= 3 counting kernels per level x <= kMaxGrid blocks
  slabF_.alloc((size_t)3 * kMaxGrid * 64 * maxW_ * sizeof(uint32_t));
  slabE_.alloc((size_t)3 * kMaxGrid * 64 * maxW_ * sizeof(unsigned long long));
  hctr_ = std::make_unique<PinnedBuf>(sizeof(Ctr));
  hsmall_ = std::make_unique<PinnedBuf>(small_.bytes);
  bctr_.alloc((size_t)(kBatch + 1) * (sizeof(Ctr) + 16 * sizeof(uint64_t)));
  hbctr_ = std::make_unique<PinnedBuf>((size_t)(kBatch + 1) * sizeof(Ctr));
  MSBFS_HIP_CHECK(hipDeviceSynchronize());
}

void BitparSolver::run(int64_t K, const int64_t* qoff, const int32_t* qids, int64_t* F,
                       int64_t* edges2, const RunOutputs& out, RunStats* st, hipStream_t stream) {
  const RunOutputs::Kind kind = out.kind(edges2 != nullptr);
  out.validate(g_.n);
  if (kind == RunOutputs::kProfile && out.nbins > INT32_MAX / 2) fail("run_profile: too many bins");
  const bool matrices = kind == RunOutputs::kDist || kind == RunOutputs::kParents;
  const bool parents = kind == RunOutputs::kParents;
  // (cleared however the run ends: a later run must launch and count nothing of this one)
  struct Scope {
    BitparSolver& b;
    ~Scope() {
      b.rec_ = Record{};
      b.pout_ = RunOutputs{};
      b.prof_ = Prof{};
    }
  } scope{*this};
  const int64_t n = g_.n;
  const int mw = std::min(maxW_, opt.max_words);
  const size_t n1 = (size_t)std::max<int64_t>(n, 1);
  if (kind == RunOutputs::kProfile) pout_ = out;
  if (matrices) {
    rec_.out = out.dist;
    rec_.ld = out.ld;
    rec_.new2old = n2o_.get(g_, stream);
    if (rec_.new2old && n > 0) {
      // (zeroed per run: a run that failed half way may have left marks)
      rslot_.ensure((size_t)n * sizeof(int32_t));
      MSBFS_HIP_CHECK(hipMemsetAsync(rslot_.p, 0, (size_t)n * sizeof(int32_t), stream));
      rec_.slot = rslot_.as<int32_t>();
    }
  }
  if (parents) {
    seen_.ensure(n1 * mw * sizeof(uint64_t));
    rec_.parent = out.parent;
    rec_.seen = seen_.as<uint64_t>();
    wq_.ensure(16 + n1 * sizeof(int32_t));
    // (zeroed per run: a run that failed half way may have left a count)
    MSBFS_HIP_CHECK(hipMemsetAsync(wq_.p, 0, 16, stream));
    rec_.wcnt = wq_.as<uint32_t>();
    rec_.wq = wq_.as<int32_t>() + 4;
  }
  // the edge-counting instantiation: asked for, or a distance run (bitpar/record.hpp)
  const bool count = edges2 != nullptr || opt.count_edges || matrices;
  const int64_t builds0 = plen_builds_;
  for (Batch b = batch_at(K, 0, mw); b.k0 < K; b = batch_at(K, b.k0 + b.nb, mw)) {
    rec_.k0 = b.k0;
    rec_.nb = b.nb;
    // the -1 fill of the pass's rows, columns [0, n) only
    for (int32_t* m : {out.dist, out.parent}) {
      if (!m || n <= 0) continue;
      int32_t* rows = m + b.k0 * out.ld;
      if (out.ld == n)
        MSBFS_HIP_CHECK(hipMemsetAsync(rows, 0xFF, (size_t)b.nb * n * sizeof(int32_t), stream));
      else
        MSBFS_HIP_CHECK(hipMemset2DAsync(rows, (size_t)out.ld * sizeof(int32_t), 0xFF,
                                         (size_t)n * sizeof(int32_t), (size_t)b.nb, stream));
    }
    // (the batch's seen rows: b.w words per vertex)
    if (parents) MSBFS_HIP_CHECK(hipMemsetAsync(seen_.p, 0, n1 * b.w * sizeof(uint64_t), stream));
    run_batch(b.w, count, b.k0, b.nb, qoff, qids, F + b.k0, edges2 ? edges2 + b.k0 : nullptr, st,
              stream);
    if (st) st->batches++;
  }
  if (st) st->builds += plen_builds_ - builds0;
}

// ---- level profiles -----------------------------------------------------------------------------
// The end of a profile batch, one thread per group: reach = the sum of its histogram rows, the
// eccentricity from far[] or, without a level >= kProfExact, the last of the exact rows with a
// count (after the leaf fold's corrections), and the histogram capped at nbins columns (rows from
// nbins - 1 on summed into the tail), group-major. res: reach[nb], ecc[nb] (as int64), then
// nb x nbins counts.
static __global__ __launch_bounds__(kBlock) void k_profile_finish(const Prof p, int rows,
                                                                  int stride, int64_t nb,
                                                                  int64_t nbins, long long* res) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= nb) return;
  long long* h = res + 2 * nb + k * nbins;
  unsigned long long reach = 0, tail = 0;
  for (int L = 0; L < rows; ++L) {
    const unsigned long long c = p.hist[(size_t)L * stride + k];
    reach += c;
    if (L < nbins - 1) h[L] = (long long)c;
    else tail += c;
  }
  if (nbins > 0) h[nbins - 1] = (long long)tail;
  long long e = (long long)p.far[k];
  if (e == 0) {
    e = -1;
    for (int L = 0; L < (int)kProfExact; ++L)
      if (p.hist[(size_t)L * stride + k]) e = L;
  }
  res[k] = (long long)reach;
  res[nb + k] = e;
}

void BitparSolver::prof_reserve(int w, int64_t nbins) {
  const size_t g = (size_t)64 * w;
  prof_buf_.ensure(64 * 16 * sizeof(uint32_t) + (size_t)prof_rows(nbins) * g * sizeof(uint64_t));
  const size_t rb = (2 + (size_t)nbins) * g * sizeof(int64_t);
  prof_res_.ensure(rb);
  if (!hprof_ || hprof_->bytes < rb) hprof_ = std::make_unique<PinnedBuf>(rb);
}

template <int W>
void BitparSolver::prof_begin(hipStream_t s) {
  prof_ = Prof{};
  if (pout_.asked != RunOutputs::kProfile) return;
  prof_reserve(W, pout_.bins());
  const int64_t rows = prof_rows(pout_.bins());
  MSBFS_HIP_CHECK(hipMemsetAsync(
      prof_buf_.p, 0, 64 * 16 * sizeof(uint32_t) + (size_t)rows * 64 * W * sizeof(uint64_t), s));
  prof_.far = prof_buf_.as<uint32_t>();
  prof_.hist = (unsigned long long*)(prof_.far + 64 * 16);
  prof_.last = (uint32_t)(rows - 1);
}

template <int W>
void BitparSolver::prof_finish(int64_t nb, hipStream_t s) {
  if (!prof_.hist) return;
  k_profile_finish<<<grid_for(nb, kBlock), kBlock, 0, s>>>(
      prof_, (int)prof_.last + 1, 64 * W, nb, pout_.bins(), prof_res_.as<long long>());
  MSBFS_HIP_CHECK(hipGetLastError());
  MSBFS_HIP_CHECK(hipMemcpyAsync(hprof_->p, prof_res_.p,
                                 (size_t)(2 + pout_.bins()) * nb * sizeof(int64_t),
                                 hipMemcpyDeviceToHost, s));
}

void BitparSolver::prof_store(int64_t k0, int64_t nb) {
  if (!prof_.hist) return;
  const int64_t* r = hprof_->as<int64_t>();
  const int64_t nbins = pout_.bins();
  for (int64_t k = 0; k < nb; ++k) {
    if (pout_.reach) pout_.reach[k0 + k] = r[k];
    if (pout_.ecc) pout_.ecc[k0 + k] = (int32_t)r[nb + k];
    if (pout_.hist)
      std::copy(r + 2 * nb + k * nbins, r + 2 * nb + (k + 1) * nbins,
                pout_.hist + (k0 + k) * pout_.hist_ld);
  }
  prof_ = Prof{};
}

// ---- distance output (bitpar/record.hpp) --------------------------------------------------------
// Level 0: the batch's (source, local group) pairs, original ids, range-checked by start_batch.
// Duplicates store the same zero twice. out: row 0 = the batch's first group. parent != nullptr
// (a parents run): the source is its own parent, and its bit goes into seen (w words per
// vertex, internal ids) with an atomic: several pairs can share a word.
static __global__ __launch_bounds__(kBlock) void k_record_sources(
    const int32_t* pv, const int32_t* pk, int64_t np, int64_t n, int64_t nb, int32_t* out,
    int64_t ld, int32_t* parent, uint64_t* seen, const int32_t* old2new, int w) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < np;
       i += (int64_t)gridDim.x * kBlock) {
    const int32_t v = pv[i], k = pk[i];
    if (!(v >= 0 && v < n && k >= 0 && k < nb)) continue;
    out[(int64_t)k * ld + v] = 0;
    if (!parent) continue;
    parent[(int64_t)k * ld + v] = v;
    const int32_t iv = old2new ? old2new[v] : v;
    if (iv >= 0 && iv < n && (k >> 6) < w)
      atomicOr((unsigned long long*)&seen[(int64_t)iv * w + (k >> 6)], 1ull << (k & 63));
  }
}

void BitparSolver::record_sources(const int32_t* pv, const int32_t* pk, int64_t np, int w,
                                  hipStream_t s) {
  if (!rec_.out || np <= 0) return;
  k_record_sources<<<cap(grid_for(np, kBlock)), kBlock, 0, s>>>(
      pv, pk, np, g_.n, rec_.nb, rec_.out + rec_.k0 * rec_.ld, rec_.ld,
      rec_.parent ? rec_.parent + rec_.k0 * rec_.ld : nullptr, rec_.seen, g_.old2new, w);
  MSBFS_HIP_CHECK(hipGetLastError());
}

void BitparSolver::run_batch(int w, bool c, int64_t k0, int64_t nb, const int64_t* qoff,
                             const int32_t* qids, int64_t* F, int64_t* edges2, RunStats* st,
                             hipStream_t s) {
#define MSBFS_BP_CASE(WW)                                                   \
  case WW:                                                                  \
    if (c) batch_impl<WW, true>(k0, nb, qoff, qids, F, edges2, st, s);      \
    else batch_impl<WW, false>(k0, nb, qoff, qids, F, edges2, st, s);       \
    break;
  switch (w) {
    MSBFS_BP_FOR_W(MSBFS_BP_CASE)
    default: fail("bad word count");
  }
#undef MSBFS_BP_CASE
}

// per-batch reset + sources + level 0 (k_init); leaves the loop state ready for level 1
template <int W, bool COUNT>
void BitparSolver::start_batch(int64_t k0, int64_t nb, const int64_t* qoff, const int32_t* qids,
                               Loop& S, hipStream_t s) {
  const int64_t n = g_.n;
  // Rows of vertices >= n_eff (deg 0) are never read: only sources can be there, and their rows
  // are zeroed by k_zero_src_rows. vis_[1]: see k_zero_src_rows.
  const size_t vb = (size_t)std::max<int64_t>(n_eff(), 1) * W * sizeof(uint64_t);
  if (!S.lazy) MSBFS_HIP_CHECK(hipMemsetAsync(vis_[0].p, 0, vb, s));
  else if (S.cnt > 0 && S.nparts > 1)  // hybrid phase A: only the rows levels 1-2 read (see k_zero_part_rows)
    k_zero_part_rows<W><<<cap(grid_for(S.cnt * Lay<W>::G, kBlock, 8192)), kBlock, 0, s>>>(
        S.cnt, S.part, S.nparts, vis_[0].as<uint64_t>());
  MSBFS_HIP_CHECK(hipMemsetAsync(done_.p, 0, done_.bytes, s));
  MSBFS_HIP_CHECK(hipMemsetAsync(anyvis_.p, 0, anyvis_.bytes, s));
  MSBFS_HIP_CHECK(hipMemsetAsync(ctr_.p, 0, sizeof(Ctr), s));
  MSBFS_HIP_CHECK(hipMemsetAsync(small_.p, 0, small_.bytes, s));
  if (!S.fold) leaf_.rows_dirty = true;  // (this batch writes leaf rows; see LeafState)
  const Small sm = small();
  // ---- sources: (vertex, local group) pairs, out-of-range ids dropped (main.cu:49)
  std::vector<int32_t> hp, hk;
  hp.reserve(2 * (qoff[k0 + nb] - qoff[k0]));
  for (int64_t k = 0; k < nb; ++k)
    for (int64_t j = qoff[k0 + k]; j < qoff[k0 + k + 1]; ++j) {
      const int32_t v = qids[j];
      if (v >= 0 && v < n) {
        hp.push_back(v);
        hk.push_back((int32_t)k);
      }
    }
  const int64_t np = (int64_t)hp.size();
  S.nsrc = np;
  // the batch's masks and source pairs go up from one pinned staging buffer (pageable copies
  // stage through the runtime and now and then stalled a step: RMAT-26 / 1024 groups, 1 step in
  // ~10-30 took +6 ms outside the level loop, tools/step_split.py); the read_ctr below retires
  // the copies before the buffer can be rewritten
  const int64_t np1 = std::max<int64_t>(np, 1);
  const size_t hbytes = 32 * sizeof(uint64_t) + (size_t)np1 * 2 * sizeof(int32_t);
  if (!hsrc_ || hsrc_->bytes < hbytes) hsrc_ = std::make_unique<PinnedBuf>(hbytes + hbytes / 2);
  {
    // gmask = the batch's groups; alive = groups with at least one valid source (computed here:
    // an atomicOr per source pair onto 16 words serialised k_init, ~0.1 ms per batch)
    uint64_t* hm = hsrc_->as<uint64_t>();
    std::fill(hm, hm + 32, 0ull);
    for (int64_t k = 0; k < nb; ++k) hm[k >> 6] |= 1ull << (k & 63);
    for (int64_t i = 0; i < np; ++i) hm[16 + (hk[i] >> 6)] |= 1ull << (hk[i] & 63);
    MSBFS_HIP_CHECK(hipMemcpyAsync(sm.gmask, hm, 16 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    MSBFS_HIP_CHECK(hipMemcpyAsync(sm.alive[0], hm + 16, 16 * sizeof(uint64_t),
                                   hipMemcpyHostToDevice, s));
  }
  pairs_.ensure((size_t)np1 * 2 * sizeof(int32_t));
  int32_t* dpv = pairs_.as<int32_t>();
  int32_t* dpk = dpv + np1;
  if (np) {
    int32_t* hpp = reinterpret_cast<int32_t*>(hsrc_->as<uint64_t>() + 32);
    std::copy(hp.begin(), hp.end(), hpp);
    std::copy(hk.begin(), hk.end(), hpp + np1);
    MSBFS_HIP_CHECK(hipMemcpyAsync(dpv, hpp, (size_t)np1 * 2 * sizeof(int32_t),
                                   hipMemcpyHostToDevice, s));
  }
  ++epoch_;
  if (S.fold) leaf_.first.ensure((size_t)np1);  // (sized by prepare_queries before a timed run)
  if (np) {
    k_zero_src_rows<W><<<cap(grid_for(np * W, kBlock)), kBlock, 0, s>>>(
        dpv, np, g_.old2new, vis_[0].as<uint64_t>(), vis_[1].as<uint64_t>());
    MSBFS_HIP_CHECK(hipGetLastError());
    k_init<W, COUNT><<<cap(grid_for(np, kBlock)), kBlock, 0, s>>>(
        dpv, dpk, np, g_.rowptr, vis_[0].as<uint64_t>(), vis_[1].as<uint64_t>(),
        acc_[S.ac].as<uint64_t>(), stamp_.as<int32_t>(), epoch_, fl_[S.fc].as<int32_t>(),
        ctr_.as<Ctr>(), sm.E, sm.alive[0], anyvis_.as<uint32_t>(), g_.old2new,
        S.fold ? leaf_.first.as<uint8_t>() : nullptr, prof_);
    MSBFS_HIP_CHECK(hipGetLastError());
    if constexpr (!COUNT) {
      if (S.fold) leaf_sources<W>(dpv, dpk, np, s);  // (+ level 0's weighted count)
    }
    if constexpr (COUNT) record_sources(dpv, dpk, np, W, s);  // (a distance run's level 0)
  }
  const HostCtr c = read_ctr(s);  // also retires the pinned/host source copies
  S.nf = c.fl2;
  S.ef = (int64_t)c.ef2;
  S.ef0 = S.ef;
  S.ev = (int64_t)c.ev2;
  S.na = n;
  S.ea = g_.nnz;  // active estimate before the first bottom-up build
}


template <int W, bool COUNT>
void BitparSolver::levels(Loop& S, RunStats* st, hipStream_t s) {
  const Small sm = small();
  // rows n (all-zero) and n + 1 (scratch) of this word count (see bitpar/pull_full.hpp)
  for (int i = 0; i < 2; ++i)
    MSBFS_HIP_CHECK(hipMemsetAsync(vis_[i].as<uint64_t>() + (size_t)std::max<int64_t>(g_.n, 1) * W,
                                   0, 2 * W * sizeof(uint64_t), s));
  static const bool trace = getenv("MSBFS_TRACE") != nullptr;
  auto tl = std::chrono::steady_clock::now();
  HostCtr c{};
  while (S.nf > 0 && S.level < S.stop_level) {
    // direction choice (Beamer et al. SC'12, on the union frontier)
    bool& bottom_up = S.bottom_up;
    if (opt.force_dir == 1) bottom_up = false;
    else if (opt.force_dir == 2) bottom_up = S.level > 0;
    else if (!bottom_up)
      // Beamer's edge test, plus a vertex test: a pull level costs about one visit per
      // non-isolated vertex (prefix pulls, early exit), a push level one scattered atomic per
      // frontier edge, so pull once the frontier has more edges than the graph has vertices
      // (RMAT-30, 256 groups: 742 -> 294 ms/step; RMAT-26, 16 groups: 16.4 -> 9.3 ms; road
      // graphs never get there). Tuning gamma scales the vertex test (0 turns it off).
      bottom_up = (double)S.ef > (double)S.ea / alpha_eff() ||
                  (tun_.gamma > 0 && S.level >= 1 &&
                   (double)S.ef > gamma_for(S.level) * (double)extent(S));
    else bottom_up = keep_pulling((double)S.nf, (double)S.ef, (double)S.na, (double)S.ea, opt.beta,
                                  alpha_eff());
    const std::string& dirs = tun_.dirs;
    if (S.level < dirs.size() && (dirs[S.level] == 'T' || dirs[S.level] == 'B'))
      bottom_up = dirs[S.level] == 'B';
    if (S.level < S.plan.size() && (S.plan[S.level] == 'T' || S.plan[S.level] == 'B'))
      bottom_up = S.plan[S.level] == 'B';
    // low-degree graphs (road-like: thousands of small top-down levels): run a batch of levels
    // without host round trips (kernels read the frontier sizes from device counters)
    if (!bottom_up) materialize_frontier(S, s);  // (a tiled pull left only its bitmap)
    if (!bottom_up && S.skip_pending) {
      // push after a dskip pull level: restore its frontier's skipped rows
      fix_done_rows<W>(S, s);
    }
    if (!bottom_up && tun_.batch > 1 && g_.max_degree <= kSmallDeg && !trace &&
        S.level + 2 < S.stop_level && opt.force_dir != 2 && S.plan.empty() &&
        (dirs.size() <= S.level)) {
      td_batch<W, COUNT>(S, st, s);
      tl = std::chrono::steady_clock::now();
      continue;
    }
    // late pull levels (small active lists: host round trips cost more than the level itself)
    if constexpr (!COUNT) {
      if (bottom_up && !trace && bu_batch_ok<W, COUNT>(S)) {
        bu_batch<W, COUNT>(S, st, s);
        tl = std::chrono::steady_clock::now();
        continue;
      }
    }
    MSBFS_HIP_CHECK(hipMemsetAsync(ctr_.p, 0, sizeof(Ctr), s));
    MSBFS_HIP_CHECK(hipMemsetAsync(sm.alive[S.alv ^ 1], 0, 16 * sizeof(uint64_t), s));
    ++S.level;
    trace::Range range_level(bottom_up ? "bitpar L%u BU" : "bitpar L%u TD", S.level);
    // slab rows written by this level's counting kernels
    const int rows = bottom_up ? level_bu<W, COUNT>(S, s) : level_td<W, COUNT>(S, s);
    if (st) ++(bottom_up ? st->bu_levels : st->td_levels);
    if (rows) {
      const int rg = std::max(1, std::min(64, rows / 32));
      const uint32_t weight = (S.level == 1 && !S.weight_l1) ? 0u : S.level;
      k_level_reduce<W, COUNT><<<W * rg, kBlock, 0, s>>>(
          slabF<W>(0), slabE<W>(0), rows, rg, sm.F, sm.E, sm.alive[S.alv ^ 1], weight, BuGate{},
          prof_at(S.level));
      MSBFS_HIP_CHECK(hipGetLastError());
    }
    c = read_ctr(s);
    if constexpr (!COUNT) {
      if (S.fold) {
        // the level's buffer and alive mask (neither index has flipped yet: the swaps are below);
        // the new frontier's list where it is short against the parents, and a list at all
        const bool by_list = !S.fl_bitmap && (int64_t)c.fl2 * 4 < leaf_.nsmall + leaf_.nheavy;
        leaf_weigh<W>(vis_[S.cur].as<uint64_t>(), sm.alive[S.alv], S.level + 1,
                      by_list ? fl_[S.fc ^ 1].as<int32_t>() : nullptr, (int64_t)c.fl2, nullptr, s);
      }
    }
    if (S.lean_ran) {
      // (high-diameter graphs: most vertices need more than their first neighbour; once a lean
      // pass sends over a quarter of its vertices on, the batch keeps the regular pull)
      if ((int64_t)c.touched * 4 > S.nact) S.lean_off = true;
      S.lean_ran = false;
    }
    if (bottom_up) {
      S.nact = c.act2;
      S.nactw = c.actw2;
      S.na = S.nact + S.nactw;
      S.ea = (int64_t)c.eu2;
    }
    const auto t2 = std::chrono::steady_clock::now();
    const double lms = std::chrono::duration<double, std::milli>(t2 - tl).count();
    if (st) {
      LevelRec rec;
      rec.batch = (int32_t)st->batches;
      rec.level = (int32_t)S.level;
      rec.dir = bottom_up ? 'B' : 'T';
      rec.kind = bottom_up ? S.kind : 0;
      rec.nf = S.nf;
      rec.ef = S.ef;
      rec.nf_next = (int64_t)c.fl2;
      rec.active = bottom_up ? S.na : (int64_t)c.touched;
      rec.ms = lms;
      st->recs.push_back(rec);
    }
    if (trace) {
      fprintf(stderr,
              "[msbfs bp W=%d] level %u %s%c nf=%lld ef=%lld -> nf'=%lld ef'=%lld touched=%u "
              "active=%lld (wide %lld) ea=%lld ev=%lld%s  %.3f ms\n",
              W, S.level, bottom_up ? "BU" : "TD", bottom_up ? S.kind : ' ', (long long)S.nf, (long long)S.ef,
              (long long)c.fl2, (long long)c.ef2, c.touched, (long long)S.na, (long long)S.nactw,
              (long long)S.ea, (long long)(S.ev + (long long)c.ev2), S.fold ? " L" : "", lms);
    }
    tl = t2;
    S.nf = c.fl2;
    S.ef = (int64_t)c.ef2;
    S.ev += (int64_t)c.ev2;
    if (S.level == 1) S.ev_l1 = S.ev;
    S.fc ^= 1;
    S.alv ^= 1;
    if (st) st->levels++;
  }
}

template <int W, bool COUNT>
void BitparSolver::batch_impl(int64_t k0, int64_t nb, const int64_t* qoff, const int32_t* qids,
                              int64_t* Fout, int64_t* edges2, RunStats* st, hipStream_t s) {
  Loop S;
  S.fold = leaf_fold_for(COUNT, 1, false, s);
  S.cnt = extent(S);
  if constexpr (!COUNT) {
    if (S.fold) leaf_begin<W>(S, s);
  }
  // lazy: no per-batch fill of vis_[0] (n_eff * 8W bytes, ~0.8 ms on RMAT-26); the edge-counting
  // pass re-reads both rows of every new vertex (k_count_frontier), so it keeps the fill
  S.lazy = tun_.lazy && !COUNT && !fused_batches<COUNT>();
  prof_begin<W>(s);
  start_batch<W, COUNT>(k0, nb, qoff, qids, S, s);
  levels<W, COUNT>(S, st, s);
  // frontier is empty: accumulator entries were cleared by finalize / zero_acc
  if constexpr (!COUNT) {
    if (S.fold) {
      leaf_end<W>(pairs_.as<int32_t>(), S.nsrc, s);
      if (st) st->leaf_folded = n_eff() - leaf_.n_core;
    }
  }
  prof_finish<W>(nb, s);
  const unsigned long long* h = read_small(s);
  prof_store(k0, nb);
  for (int64_t k = 0; k < nb; ++k) {
    Fout[k] = (int64_t)h[k];
    if (edges2) edges2[k] = (int64_t)h[64 * 16 + k];
  }
}


#define MSBFS_BP_INST(WW)                                                                         \
  template void BitparSolver::start_batch<WW, false>(int64_t, int64_t, const int64_t*,          \
                                                     const int32_t*, Loop&, hipStream_t);        \
  template void BitparSolver::start_batch<WW, true>(int64_t, int64_t, const int64_t*,           \
                                                    const int32_t*, Loop&, hipStream_t);         \
  template void BitparSolver::levels<WW, false>(Loop&, RunStats*, hipStream_t);                 \
  template void BitparSolver::levels<WW, true>(Loop&, RunStats*, hipStream_t);
MSBFS_BP_FOR_W(MSBFS_BP_INST)
#undef MSBFS_BP_INST

// first launch of any kernel of this translation unit loads its code object (see
// load_code_objects in bitpar/solver.hpp)
static __global__ void k_load_solver() {}
void load_code_solver(hipStream_t s) {
  k_load_solver<<<1, 64, 0, s>>>();
  MSBFS_HIP_CHECK(hipGetLastError());
}

}  // namespace bp

std::unique_ptr<Solver> make_bitpar_solver(const DeviceGraph& g, int max_groups) {
  return std::make_unique<bp::BitparSolver>(g, max_groups);
}

}  // namespace msbfs
