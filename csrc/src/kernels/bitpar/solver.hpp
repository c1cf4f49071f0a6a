// Bit-parallel, direction-optimising multi-source BFS over up to 64*W query groups at once.
//
// What it replaces: the reference runs each query group as its own level-synchronous BFS with a
// thread-per-vertex kernel that rescans all n distances every level (BFSKernal main.cu:16-38,
// driven by GPUMultiSourceBFS main.cu:40-73), then copies all n distances to the host to sum them
// (ComputeFofU main.cu:75-89). Queries run strictly one after another per rank
// (main.cu:312-322).
//
// Here one pass over the graph advances 64*W groups together (MS-BFS, Then et al. VLDB'15):
//  * every vertex owns W 64-bit words: bit k of word j = "visited by group 64j+k".
//  * top-down levels (small frontiers) push frontier bits along edges with 64-bit atomicOr into
//    an accumulator, edge-parallel via a load-balanced search over the frontier's degree prefix
//    (no hub serialisation);
//  * bottom-up levels (large frontiers) pull: an unfinished vertex ORs its neighbours' visited
//    words and stops as soon as every still-alive group is covered (early exit). Double-buffered
//    visited arrays make the pull race-free without a separate frontier array (a neighbour bit
//    visited at any level <= L can only have been set exactly at L if it is still missing here).
//    Low-degree vertices get G lanes each; high-degree vertices are cut into fixed-size edge
//    chunks that many waves scan in parallel (partial ORs merged with atomicOr, then a finalize
//    pass), so a 10^6-neighbour hub never serialises a level on one wave.
//  * per-group F(U) = sum_level level * |newly visited| is accumulated on chip: every new bit adds
//    to a per-group LDS counter; one global atomic per group per block at the end. Only 8 bytes
//    per group ever leave the device (vs 4n bytes per query in the reference).
//  * groups whose frontier died are masked out ("alive" words), so groups stuck in small
//    components never stop other groups' vertices from finishing.
//  * list building (active lists, frontiers, touched sets) goes through per-block LDS queues:
//    one global atomic per ~1K items instead of one per wave (same-line atomics serialise).
// Lane mapping for wave64: each lane owns VW (1-2) words = one 8-16 B load, a vertex's W words are
// spread over G = W/VW consecutive lanes, so W=16 reads a vertex's 128-B line in one coalesced
// wave-instruction slice.
//
// Source layout (one class, five translation units that compile in parallel):
//   bitpar/bits.hpp                      pure bit helpers (HIP-free, pinned by the host self-test)
//   bitpar/common.hpp  init.hpp  push.hpp  hybrid.hpp  tiles.hpp      kernels by family; the pull
//   bitpar/pull.hpp  pull_full.hpp  pull_lists.hpp  pull_tail.hpp     levels': pulls, lists, tail push
//   bitpar/record.hpp                    the distance / parent output (RunOutputs::dist, parent), per level
//   bitpar_solver.hip  construction, run() (one batch loop, the per-kind setup off
//                      RunOutputs::kind), the level loop (direction choice, reductions)
//   bitpar_push.hip    top-down levels and the device-driven level batches
//   bitpar_pull.hip    bottom-up levels (prefix pull + tail push, narrow / lean / chunk pulls),
//                      each carried out from a plan: bitpar/pull_plan.hpp (plain host code)
//   bitpar_tiles.hip   the first pull level over static vertex tiles
//   bitpar/leaf.hpp  leaf_kernels.hpp    leaf folding: degree-1 vertices counted through their parents
//                                        (decision and lists: plain host code; launched from bitpar_pull.hip)
//   bitpar/tuning.hpp, ../bitpar_tuning.cpp   the tuning keys and their parser (plain host code)
//   bitpar_hybrid.hip  the hybrid multi-GPU phases and the exchange coding
#pragma once

#include <chrono>
#include <functional>
#include <vector>
#include <memory>
#include <string>

#include "common.hpp"
#include "leaf.hpp"
#include "pull_plan.hpp"
#include "record.hpp"

namespace msbfs {
namespace bp {

// The runtime loads a translation unit's code object on the first launch of one of its kernels:
// 1.5-2.8 ms each for the solver's units (hipLaunchKernel in a runtime trace of the first run,
// round 6), which made the first run after preparation ~4 ms slower than the next ones on
// RMAT-26 (level 1's k_init / k_td_expand came first from their units). prepare() loads them
// all, as device setup before the reference's computation phase (main.cu:282-298).
void load_code_solver(hipStream_t s);
void load_code_push(hipStream_t s);
void load_code_pull(hipStream_t s);
void load_code_hybrid(hipStream_t s);
void load_code_tiles(hipStream_t s);
inline void load_code_objects(hipStream_t s) {
  load_code_solver(s);
  load_code_push(s);
  load_code_pull(s);
  load_code_hybrid(s);
  load_code_tiles(s);
}

struct ChunkDesc;  // (bitpar/pull_lists.hpp)

class BitparSolver final : public Solver {
 public:
  BitparSolver(const DeviceGraph& g, int max_groups);

  // One batch loop for every kind of out. Distances (and parents, the first-in-row BFS parent:
  // bitpar/record.hpp) force the edge-counting instantiation; a profile (reach, eccentricity,
  // vertices per level) runs the same kernels and decisions as a plain run, the counts kept where
  // they pass on their way into F.
  void run(int64_t K, const int64_t* qoff, const int32_t* qids, int64_t* F, int64_t* edges2,
           const RunOutputs& out, RunStats* st, hipStream_t stream) override;
  void tune(const std::string& spec) override { tun_.parse(spec); }
  int64_t pass_groups() const override { return 64 * (int64_t)std::min(maxW_, opt.max_words); }
  // graph-derived tables and worst-case scratch, built before any timed run (bitpar_pull.hip)
  void prepare(hipStream_t s) override;
  void prepare_hybrid(int part, int nparts, hipStream_t s) override;
  void prepare_queries(int64_t K, const int64_t* qoff, const int32_t* qids,
                       hipStream_t s) override;

  int64_t hybrid_max_groups() const override { return 64 * (int64_t)maxW_; }
  void hybrid_phase_a(int64_t K, const int64_t* qoff, const int32_t* qids, int part, int nparts,
                      int64_t n_eff, bool count_l1, const int32_t* wbeg, uint64_t* send,
                      int64_t* out, RunStats* st, hipStream_t s, int64_t* coded_len = nullptr,
                      int chunks = 1, ChunkFn cb = nullptr, void* user = nullptr) override;
  void hybrid_chunk_bounds(int part, int nparts, int64_t n_eff, int chunks, int64_t* bounds,
                           hipStream_t s) override;
  void hybrid_phase_c(int64_t K, int w_begin, int w_count, int nparts, int64_t n_eff,
                      const uint64_t* recv, const int64_t* reduced, int64_t* F_out, RunStats* st,
                      hipStream_t s) override;
  void hybrid_decode(const uint64_t* coded, const int64_t* coded_len, int nparts, int64_t n_eff,
                     int w_count, uint64_t* dense, hipStream_t s) override;

  // Level-loop state. The normal path runs one batch start to finish; the hybrid phases run
  // a capped / range-restricted piece of it (phase A) or resume it from exchanged state (C).
  struct Loop {
    int cur = 0;  // vis_[cur] = read buffer (up to date for every non-done vertex)
    int fc = 0;   // fl_[fc] = current frontier
    int ac = 0;   // acc_[ac] holds the current frontier bits when fsrc_acc
    int alv = 0;  // alive[alv] = groups with a non-empty frontier
    uint32_t level = 0;
    int64_t nf = 0, ef = 0, ev = 0, na = 0, ea = 0, nact = 0, nactw = 0;
    int64_t nsrc = 0;  // the batch's (source, group) pairs
    bool have_active = false, fsrc_acc = true, bottom_up = false;
    int bu_levels = 0;
    // limits
    uint32_t stop_level = 0xFFFFFFFFu;  // last level to run
    int64_t cnt = 0;                    // first active-list build: v = part + i*nparts, i < cnt
    int part = 0, nparts = 1;
    bool weight_l1 = true;              // add level-1 counts to F
    std::string plan;                   // plan[level] = 'T'/'B' forces the next level
    int64_t ev_l1 = 0;                  // ev after level 1
    int64_t ef0 = 0;                    // degree sum of the sources (level-0 frontier)
    bool lazy = false;                  // no vis_[0] fill (see start_batch)
    bool osnap_next = false;            // the previous level was the first pull of a lazy batch
    bool lean_off = false;              // a lean first-row pass overflowed (see k_bu_first)
    bool lean_ran = false;              // this level ran one (its overflow count is c.touched)
    bool old_stale = false;             // k_td_fused levels updated only vis_[cur]
    bool fl_bitmap = false;             // fl_[fc] not built yet: the frontier is in fbm_tile_
    // chunked hybrid phase A: the tiled level-2 pull runs the own-vertex ranges
    // [chunk_b[c], chunk_b[c+1]) one after another and calls on_chunk(c) after each (its rows
    // are final then); chunks_done counts the calls (phase A makes up the rest after the level)
    std::vector<int64_t> chunk_b;
    std::function<void(int)> on_chunk;
    int chunks_done = 0;
    // dskip: the last level skipped the rows of the vertices it finished; a push level next
    // restores those of its frontier (k_fix_done_rows) from the read buffer and this alive mask
    bool keep_rows = false;
    bool push_after = false;  // this tiled level's tail push runs after the tiles (k_push_tail_after)
    bool skip_pending = false;
    const uint64_t* skip_alive = nullptr;
    // a level skipped rows: every later pull level of the batch probes dsnap_ (re-snapshotted
    // at the start of the first pull level after each skipping level)
    bool skipped_any = false, resnap = false;
    char kind = 0;  // the last pull level's PullPlan::kind (its level record's)
    bool fold = false;  // leaf folding (bitpar/leaf.hpp): the traversal ends at leaf_.n_core
  };
  struct Small {
    unsigned long long* F;
    unsigned long long* E;
    uint64_t* alive[2];
    uint64_t* gmask;
  };

 private:
  Small small() {
    Small r;
    r.F = small_.as<unsigned long long>();
    r.E = r.F + 64 * 16;
    r.alive[0] = (uint64_t*)(r.E + 64 * 16);
    r.alive[1] = r.alive[0] + 16;
    r.gmask = r.alive[1] + 16;
    return r;
  }
  template <int W>
  uint32_t* slabF(int row) { return slabF_.as<uint32_t>() + (size_t)row * 64 * W; }
  template <int W>
  unsigned long long* slabE(int row) {
    return slabE_.as<unsigned long long>() + (size_t)row * 64 * W;
  }

  // ---- bitpar_solver.hip
  template <int W, bool COUNT>
  void start_batch(int64_t k0, int64_t nb, const int64_t* qoff, const int32_t* qids, Loop& S,
                   hipStream_t s);
  template <int W, bool COUNT>
  void levels(Loop& S, RunStats* st, hipStream_t s);
  template <int W, bool COUNT>
  void batch_impl(int64_t k0, int64_t nb, const int64_t* qoff, const int32_t* qids, int64_t* F,
                  int64_t* edges2, RunStats* st, hipStream_t s);
  void run_batch(int w, bool count, int64_t k0, int64_t nb, const int64_t* qoff,
                 const int32_t* qids, int64_t* F, int64_t* edges2, RunStats* st, hipStream_t s);
  // ---- bitpar_push.hip: one top-down level (returns the counter-slab rows it wrote)
  template <int W, bool COUNT>
  int level_td(Loop& S, hipStream_t s);
  template <int W, bool COUNT>
  void td_batch(Loop& S, RunStats* st, hipStream_t s);
  // ---- bitpar_pull.hip: one bottom-up level (returns the counter-slab rows it wrote)
  template <int W, bool COUNT>
  int level_bu(Loop& S, hipStream_t s);
  // One pull level in flight: its plan and what the stages hand on to each other.
  struct BuLevel {
    PullPlan p;
    const uint64_t* R;      // read buffer vis_[cur]
    uint64_t* O;            // the other one, written
    const uint64_t* alive;
    Small sm;
    int rows = 0;           // slab rows written by this level's counting kernels so far
    int32_t H = kPfxH;      // prefix bound (see pfx_bound)
    const uint32_t* snap = nullptr;    // any-visited snapshot of a lazy batch's first pull
    const uint32_t* dsnap = nullptr;   // done snapshot (done_probe), probed where p.probe
    const uint32_t* dprobe = nullptr;
    const uint32_t* codes = nullptr;   // sparse row codes from code_from on
    int32_t code_from = INT32_MAX;     // (kNoCodes)
    const int32_t* plen = nullptr;     // prefix lengths of the per-vertex prefix pull
  };
  PlanGraph plan_graph() {
    return PlanGraph{g_.n, n_eff(), g_.nnz, g_.rows_sorted, g_.old2new != nullptr, full_pull()};
  }
  PlanLevel plan_level(const Loop& S) const;
  // the stages of level_bu, in order
  void bu_build_lists(Loop& S, BuLevel& L, hipStream_t s);
  void bu_snapshots(Loop& S, BuLevel& L, hipStream_t s);
  template <int W>
  void bu_codes(Loop& S, BuLevel& L, hipStream_t s);
  template <int W>
  void bu_tail_push(Loop& S, BuLevel& L, hipStream_t s);
  template <int W, bool COUNT>
  void bu_narrow(Loop& S, BuLevel& L, hipStream_t s);
  template <int W>
  void bu_chunks(Loop& S, BuLevel& L, const ChunkDesc* d, const int64_t* np, int64_t maxc,
                 hipStream_t s);
  template <int W, bool COUNT>
  void bu_wide(Loop& S, BuLevel& L, hipStream_t s);
  // the one host-side launcher of k_bu_narrow / k_bu_full (any instantiation `k`)
  struct PullArgs {
    const int32_t* list;
    int64_t nact;
    const uint64_t* R;
    uint64_t* O;
    const uint64_t* alive;
    int32_t *act2, *actw2, *fl2;
    Ctr* ctr;
    uint32_t* slab;
    // optional
    int32_t filter_from = INT32_MAX;  // (k_bu_narrow)
    uint64_t* pacc = nullptr;
    const int32_t* stamp = nullptr;
    int32_t epoch = 0;
    const int32_t* plen = nullptr;
    const uint32_t* nact_dev = nullptr;
    const uint32_t* snap = nullptr;
    BuGate gate{};
    const uint32_t* dprobe = nullptr;  // (k_bu_full)
    int flags = 0;
  };
  // (Cfg: a k_bu_narrow variant, bitpar/pull.hpp; p: the level's plan, whose launch shape the
  // variant must have)
  template <int W, class Cfg>
  void launch_narrow(int grid, const PullArgs& a, hipStream_t s, const PullPlan* p = nullptr);
  template <class K>
  void launch_full(K k, int grid, const PullArgs& a, hipStream_t s);
  template <int W, bool COUNT>
  bool bu_batch_ok(const Loop& S) {
    PlanLevel l = plan_level(S);
    l.forced = !S.plan.empty() || tun_.dirs.size() > S.level;
    return pull_batch_ok(plan_graph(), tun_, COUNT, l);
  }
  template <int W, bool COUNT>
  void bu_batch(Loop& S, RunStats* st, hipStream_t s);
  const int32_t* prefix_lens(int32_t H, hipStream_t s);
  // the cached prefix lengths if they are for bound H (and these graph buffers), else nullptr
  const int32_t* cached_prefix_lens(int32_t H) const {
    return (plen_key_[0] == (const void*)g_.rowptr && plen_key_[1] == (const void*)g_.col &&
            plen_h_ == H)
               ? plen_.as<int32_t>()
               : nullptr;
  }
  int64_t plen_builds_ = 0;  // prefix-length builds so far (a run reports its own: RunStats::builds)
  template <int W>
  int32_t pfx_bound(const Loop& S) { return pfx_bound_n(W, S.nsrc); }
  int32_t pfx_bound_n(int W, int64_t nsrc);  // prefix bound of the untiled prefix level
  // ---- bitpar_tiles.hip: the first pull level's prefix pull over static vertex tiles
  struct TileSet {
    DevBuf pent, tiles, big;
    int64_t ntiles = 0, nbig = 0, nent = 0;
    int64_t t_core = 0;  // tiles of the ids < leaf_n_core() (a tile ends there; part 0 of 1)
    std::vector<int64_t> ti, te;  // host: own-vertex index and first entry of every tile (+ end)
    int64_t last_partial = -1;    // last tile of a big vertex (they all precede chunk 1)
    int part = -1, nparts = 0;
    const void* key[2] = {nullptr, nullptr};
  };
  // the tiles of the own vertices (part of nparts; built on first use and cached per graph
  // buffers; nullptr for fewer than 8 words, or when they do not fit in HBM)
  const TileSet* pfx_tiles(int W, int part, int nparts, hipStream_t s);
  // some word count of this solver may take the tiled first pull level (the graph-side half of
  // wants_tiles; pfx_tiles adds the word-count half: W >= 4 and W >= tiles_w)
  bool tiles_possible() {
    return tun_.tiles && prefix_capable(plan_graph(), tun_) && maxW_ >= 4 && maxW_ >= tun_.tiles_w;
  }
  template <int W>
  int tiles_pull(Loop& S, hipStream_t s, const uint64_t* R, uint64_t* O, const uint32_t* snap,
                 const uint32_t* codes, int32_t code_from, int rows);
  // the frontier list of a tiled level is only a bitmap until a top-down level needs it
  void materialize_frontier(Loop& S, hipStream_t s);
  const int32_t* first_nbr(hipStream_t s);
  int32_t code_bound(double min_deg);
  // ---- bitpar_hybrid.hip
  template <int W>
  void phase_a_impl(int64_t K, const int64_t* qoff, const int32_t* qids, int part, int nparts,
                    int64_t n_eff, bool count_l1, const int32_t* wbeg, uint64_t* send,
                    int64_t* out, RunStats* st, hipStream_t s, int64_t* coded_len, int chunks,
                    ChunkFn cb, void* user);
  template <int W>
  void phase_c_impl(int64_t K, int w_begin, int w_count, int nparts, int64_t n_eff,
                    const uint64_t* recv, const int64_t* reduced, int64_t* F_out, RunStats* st,
                    hipStream_t s);
  template <int W>
  void code_send(const uint64_t* vis, uint64_t* staging, int64_t cnt, int part, int nparts,
                 const int32_t* wbeg, uint64_t* send, int64_t* coded_len, hipStream_t s);
  // scratch of the exchange coding: bitmap words, popcounts and their inclusive scan per chunk
  struct CodeWs {
    uint64_t* bits;
    int64_t* pop;
    int64_t* incl;
    void* tmp;
    size_t tmp_bytes;
  };
  CodeWs code_ws(int64_t chunks);

  // device-driven top-down batches run k_td_fused levels (needs every row of vis_[cur] valid,
  // i.e. no lazy batch; the edge-counting pass keeps expand + finalize + k_count_frontier)
  double alpha_eff() const {
    return fused_batches<false>() ? std::min(opt.alpha, kAlphaLow) : opt.alpha;
  }
  template <bool COUNT>
  bool fused_batches() const {
    return !COUNT && tun_.td_fused && tun_.batch > 1 && g_.max_degree <= kSmallDeg &&
           (double)g_.nnz <= kTdFusedDeg * (double)std::max<int64_t>(g_.n, 1);
  }
  // push -> pull test threshold on the frontier's degree sum for the level after `done_levels`
  // completed ones (the vertex half of the direction test, see levels())
  // gamma2 (the earlier pull at level 2) only on skewed graphs (max degree > 16x the mean): there
  // the level-1 frontier holds hubs and the prefix pull covers most edges cheaply. On a uniform
  // random graph (n = 16M, m = 128M, 1024 groups, ef / n_eff = 0.26 at level 2) it pulled where a
  // push was 2.5 ms cheaper (34.2 vs 29.1 ms per step, round 4).
  double gamma_for(uint32_t done_levels) {
    if (done_levels != 1 || tun_.gamma2 < 0) return tun_.gamma;
    if (!tun_.gamma2_auto) return tun_.gamma2;  // (set explicitly: applies to every graph)
    const double mean = (double)g_.nnz / (double)std::max<int64_t>(n_eff(), 1);
    return (double)g_.max_degree > 16.0 * mean ? tun_.gamma2 : tun_.gamma;
  }

  // ---- leaf folding (bitpar/leaf.hpp; bitpar_pull.hip)
  struct LeafState {
    const void* key[3] = {nullptr, nullptr, nullptr};  // the graph buffers the tables are for
    bool bounds = false, lists = false;                // n_core known / the lists are built
    bool no_room = false;                              // ... or did not fit: runs stay unfolded
    int64_t n_core = 0, parents = 0, attached = 0, max_w = 0, nsmall = 0, nheavy = 0;
    DevBuf plist, pw, pidx, seen, epoch, first;
    // Leaf rows are written by k_init alone while folding, so in both visited buffers they must be
    // all zero or the batch's source bits: a folded batch zeroes its source rows again at its
    // end, and the first one after anything else (an unfolded batch, another word count) zeroes
    // the whole leaf range.
    bool rows_dirty = true;
    int rows_w = 0;
  };
  LeafState leaf_;
  int32_t leaf_epoch_ = 0;
  // first id of degree <= 1 (n_eff() where the ids are not in degree order)
  int64_t leaf_n_core();
  // is this run folded? builds the lists on first use (prepare() does it before any timed run)
  bool leaf_fold_for(bool count, int nparts, bool limited, hipStream_t s);
  void leaf_build(hipStream_t s);
  template <int W>
  void leaf_begin(Loop& S, hipStream_t s);  // before start_batch
  template <int W>
  void leaf_sources(const int32_t* pv, const int32_t* pk, int64_t np, hipStream_t s);
  template <int W>
  void leaf_end(const int32_t* pv, int64_t np, hipStream_t s);
  // The weighted count of one level (weight = level + 1) after its kernels: R = the buffer the
  // level wrote, alive = the mask its kernels used. The new frontier's list (n entries, or *n_dev)
  // where that is short, else (list == nullptr) every parent.
  template <int W>
  void leaf_weigh(const uint64_t* R, const uint64_t* alive, uint32_t weight, const int32_t* list,
                  int64_t n, const uint32_t* n_dev, hipStream_t s);
  // vertices a folded run's traversal covers (else every non-isolated one)
  int64_t extent(const Loop& S) { return S.fold ? leaf_.n_core : n_eff(); }
  int32_t push_bound(const Loop& S) const { return S.fold ? (int32_t)leaf_.n_core : INT32_MAX; }

  // 1 + the last vertex with deg > 0 (cached per graph buffers: relabelling replaces them).
  // Vertices beyond it are never active, never neighbours: level loops and clears skip them.
  int64_t n_eff() {
    if (eff_key_[0] != (const void*)g_.rowptr || eff_key_[1] != (const void*)g_.col ||
        eff_key_[2] != (const void*)g_.old2new) {
      n_eff_ = hybrid_extent(g_);
      eff_key_[0] = g_.rowptr;
      eff_key_[1] = g_.col;
      eff_key_[2] = g_.old2new;
    }
    return n_eff_;
  }


  HostCtr read_ctr(hipStream_t s) {
    MSBFS_HIP_CHECK(hipMemcpyAsync(hctr_->p, ctr_.p, sizeof(Ctr), hipMemcpyDeviceToHost, s));
    MSBFS_HIP_CHECK(hipStreamSynchronize(s));
    const Ctr* c = hctr_->as<Ctr>();
    return HostCtr{c->act2.v, c->actw2.v, c->fl2.v, c->touched.v, c->ef2.v, c->eu2.v, c->ev2.v};
  }

  // copy the small block (F, E, alive, gmask) to pinned host memory and wait
  const unsigned long long* read_small(hipStream_t s) {
    MSBFS_HIP_CHECK(hipMemcpyAsync(hsmall_->p, small_.p, small_.bytes, hipMemcpyDeviceToHost, s));
    MSBFS_HIP_CHECK(hipStreamSynchronize(s));
    return hsmall_->as<unsigned long long>();
  }

  // ---- fixed policy constants (formerly environment knobs; measured, see README)
  static constexpr int kTdGrid = 1024;        // blocks of the device-driven batches' kernels
  static constexpr int64_t kTdWideFrontier = 393216;  // (one word: 5 blocks per CU from here)
  static constexpr int kTdRed = 6;            // fused levels per k_level_reduce_multi launch
  // push -> pull threshold (Beamer's alpha) on graphs with max degree <= kSmallDeg (fused
  // top-down levels). Road grid 4896^2, 256 groups: alpha 14 pulls from ~1.7M frontier vertices
  // on and takes 3030 ms, alpha 4 stays top-down (1648 ms batched)
  static constexpr double kAlphaLow = 4.0;
  // fused levels only below this mean degree (road-like graphs): denser low-degree graphs pull
  // after a few levels (uniform n = 16M, m = 128M, 1024 groups: 29.6 ms vs 32.3 ms fused)
  static constexpr double kTdFusedDeg = 8.0;
  static constexpr int kBatch = 64;  // most levels per device-driven batch
  bool full_pull() const { return full_pull_ok(tun_, g_.n); }

  const DeviceGraph& g_;
  Tuning tun_;
  int maxW_ = 1;
  DevBuf vis_[2], acc_[2], stamp_, done_, act_[2], actw_[2], fl_[2], touched_, offs_, scan_tmp_,
      ctr_, small_, pairs_, slabF_, slabE_, anyvis_, desc_;
  size_t scan_bytes_ = 0;
  std::unique_ptr<PinnedBuf> hctr_, hsmall_, hsrc_;  // (hsrc_: start_batch's H2D staging)
  int32_t epoch_ = 0;
  int64_t n_eff_ = 0;
  const void* eff_key_[3] = {nullptr, nullptr, nullptr};
  DevBuf plen_;
  DevBuf chunk_cnt_;  // pass-1 chunk count of the two-pass wide pull (device int64)
  DevBuf first_;
  DevBuf code_ws_;
  const void* first_key_[2] = {nullptr, nullptr};
  bool first_ok_ = true;  // the first-neighbour array fits (RMAT-30: no room; col[rowptr[v]])
  const void* plen_key_[2] = {nullptr, nullptr};
  int32_t plen_h_ = 0;
  DevBuf fbm_[2];   // frontier bitmaps of the fused levels (n bits each)
  DevBuf asnap_;    // any-visited bitmap at the start of a lazy batch's first pull level
  std::vector<int32_t> deg_bounds_;  // first id with degree < 2^k (relabelled graphs)
  const void* code_key_[2] = {nullptr, nullptr};
  int batch_next_ = 4;  // levels of the next device-driven batch (doubles while the frontier lives)
  int bu_next_ = 4;     // levels of the next device-driven pull batch (the last run's pull tail + 1)
  std::vector<std::unique_ptr<TileSet>> tilesets_;  // per vertex partition (hybrid emulation: all)
  bool tiles_ok_ = true;  // false once the tiles did not fit
  DevBuf fbm_tile_, lcnt_, zrow_;  // frontier bitmap of a tiled level, list counter, zero row
  DevBuf dsnap_;                   // done bitmap as of a dskip level's start
  // dskip: the done-bitmap snapshot a pull level probes (nullptr: no probes); skip_now: this
  // level skips the rows of the vertices it finishes
  const uint32_t* done_probe(Loop& S, bool skip_now, hipStream_t s);
  template <int W>
  void fix_done_rows(Loop& S, hipStream_t s);
  int num_cus_ = 0;
  // Blocks of a k_bu_full launch: one lane per vertex (<= 2 words) runs five waves per SIMD
  // (96 VGPRs), so 5 blocks per CU are resident; the 2048-block cap then ran a second round with
  // 768 blocks on every level (a grid-stride loop hands every block the same work). Capped
  // below 2^27 list entries only: RMAT-26 level 3 at 64 / 128 groups ~1.58 -> 1.50 / ~2.87 ->
  // 2.80 ms, but RMAT-30 at 32 groups (~2^29 entries) 20.15 -> 20.65 ms with the cap. From 4
  // words (four waves per SIMD, 4 blocks per CU resident) only the device-driven batches (batch:
  // lists <= bu_max, each block's fixed epilogue of counters and list atomics dominates) take
  // the resident grid: RMAT-26 / 1024 groups levels 5-7 0.070-0.072 -> 0.060-0.063 ms each
  // (2 or 3 blocks per CU: 0.059-0.060); level 3 with it ran 5.20 -> 5.26-5.32 ms.
  template <int W>
  int full_grid(int g, int64_t nact, bool batch = false) {
    if (nact >= (int64_t{1} << 27)) return g;
    const int cus = std::max(1, num_cus());
    if (Lay<W>::VPW == 64) return std::min(g, 5 * cus);
    return batch ? std::min(g, 4 * cus) : g;
  }
  // the block count of a grid-stride level kernel under the test key max_grid (0: unchanged)
  int cap(int grid) const { return grid_capped(grid, tun_.max_grid); }
  int num_cus() {  // (compute units of the solver's GPU, queried once)
    if (num_cus_ == 0) {
      hipDeviceProp_t prop;
      MSBFS_HIP_CHECK(hipGetDeviceProperties(&prop, g_.device));
      num_cus_ = prop.multiProcessorCount;
    }
    return num_cus_;
  }
  DevBuf bctr_;  // (kBatch+1) Ctr slots, then (kBatch+1) x 16 alive words
  // ---- distance output (bitpar/record.hpp)
  Record rec_;     // set by a distance run for its duration; rec_.out == nullptr otherwise
  InverseMap n2o_;  // inverse of g_.old2new, built on first use, cached per map
  DevBuf rslot_;   // the dense walk's marks (record.hpp), n int32, zero between levels
  DevBuf seen_;    // a parents run's seen rows (record.hpp), n * W words, zeroed per batch
  DevBuf wq_;      // its wide queue: a counter (first 16 bytes), then n vertex ids
  // the level-0 zeros of a batch's source pairs / one level's new bits off the new frontier list
  // fl_[fc ^ 1] (length from ctr; new bits = a, or a & ~b with DIFF), right after the level's
  // k_count_frontier. Both launch nothing unless a distance run is under way; in a parents run
  // (rec_.parent) they also store the parents: the sources' own ids, and per level the search
  // against the seen rows that entered the level (narrow vertices, then the queued wide ones),
  // then the commit of the level's bits to them.
  void record_sources(const int32_t* pv, const int32_t* pk, int64_t np, int w, hipStream_t s);
  template <int W, bool DIFF>
  void record_level(const int32_t* fl, const Ctr* ctr, const uint64_t* a, const uint64_t* b,
                    int64_t nmax, int grid_cap, uint32_t level, hipStream_t s,
                    bool may_dense = true) {
    if (!rec_.out) return;
    // (nmax bounds the list's length; the dense walk only where the list can be large)
    const bool dense = may_dense && rec_.slot && nmax * kRecordDenseDiv >= g_.n;
    if (dense)
      k_record_mark<<<grid_for(nmax, kBlock, grid_cap), kBlock, 0, s>>>(fl, ctr, rec_.new2old,
                                                                        g_.n, rec_.slot);
    k_record_levels<W, DIFF><<<grid_for(dense ? g_.n : nmax, kBlock, grid_cap), kBlock, 0, s>>>(
        fl, ctr, a, b, rec_.new2old, dense ? rec_.slot : nullptr, g_.n,
        rec_.out + rec_.k0 * rec_.ld, rec_.ld, rec_.nb, (int32_t)level);
    MSBFS_HIP_CHECK(hipGetLastError());
    if (!rec_.parent) return;
    k_record_parents<W, DIFF><<<grid_for(nmax, Lay<W>::TILE, grid_cap), kBlock, 0, s>>>(
        fl, ctr, a, b, g_.rowptr, g_.col, rec_.seen, rec_.new2old, g_.n,
        rec_.parent + rec_.k0 * rec_.ld, rec_.ld, rec_.nb, rec_.wq, rec_.wcnt);
    // (the queue's length is known on the device only: a block per queued vertex, grid-stride;
    // no launch on a graph that has no wide vertex, so none in the device-driven push batches)
    if (g_.max_degree >= kRecordWideDeg)
      k_record_parents_wide<W, DIFF><<<grid_for(nmax, 1, grid_cap), kBlock, 0, s>>>(
          rec_.wq, rec_.wcnt, a, b, g_.rowptr, g_.col, rec_.seen, rec_.new2old, g_.n,
          rec_.parent + rec_.k0 * rec_.ld, rec_.ld, rec_.nb);
    k_record_commit<W, DIFF><<<grid_for(nmax * W, kBlock, grid_cap), kBlock, 0, s>>>(
        fl, ctr, a, b, g_.n, rec_.seen, rec_.wcnt);
    MSBFS_HIP_CHECK(hipGetLastError());
  }
  std::unique_ptr<PinnedBuf> hbctr_;
  // ---- level profiles (Prof in bitpar/common.hpp)
  // What a profile run asked for (whole run; a batch writes its groups' part), plain otherwise
  RunOutputs pout_;
  Prof prof_;  // the current batch's device counts; prof_.hist == nullptr outside a profile run
  // far[64 * 16], then the histogram rows (rows x 64 * W of the batch); the batch's results
  // (reach, ecc, the capped histogram group-major) on the device and in pinned memory
  DevBuf prof_buf_, prof_res_;
  std::unique_ptr<PinnedBuf> hprof_;
  static constexpr int64_t kProfBins = 64;  // the bins prepare() sizes the buffers for
  static int64_t prof_rows(int64_t nbins) { return std::max<int64_t>(nbins, kProfExact + 1); }
  void prof_reserve(int w, int64_t nbins);
  Prof prof_at(uint32_t level) const {
    Prof p = prof_;
    p.level = level;
    return p;
  }
  template <int W>
  void prof_begin(hipStream_t s);  // before start_batch: zeroed counts
  // after the batch's last kernel: results -> pinned memory (enqueued; read_small waits) ...
  template <int W>
  void prof_finish(int64_t nb, hipStream_t s);
  void prof_store(int64_t k0, int64_t nb);  // ... and from there to the caller's arrays
};

// explicit instantiation of a member template for every word count (W) and counting mode
#define MSBFS_BP_FOR_W(X) X(1) X(2) X(4) X(8) X(16)

}  // namespace bp
}  // namespace msbfs
