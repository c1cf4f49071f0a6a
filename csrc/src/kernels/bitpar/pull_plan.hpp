// The plan of one bottom-up (pull) level of the bit-parallel solver: every decision level_bu
// takes (which kernels, which variants, which scheduling), computed by plain host code from the
// graph's facts, the options, the tuning and the level loop's state. No HIP here: the host self
// test (csrc/tests/host_selftest.cpp) pins the decisions without a GPU. BitparSolver::level_bu
// (bitpar_pull.hip) only carries a plan out.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>

#include "tuning.hpp"

namespace msbfs {
namespace bp {

// Probes of the lowest ids (the hubs after degree relabelling) read an LDS copy of their
// any-visited bitmap words: kHubW words = 56 KB (ids < 458752, two blocks per CU) or, where one
// 1024-thread block per CU has the LDS to itself, kHubBig words = 128 KB (ids < 1M).
constexpr int kHubW = 14336, kHubBig = 32768;
// Prefix pull + tail push on the first bottom-up level (see k_push_tail): the pulls stop at the
// small hub bitmap's bound H = 458752 (RMAT-26 level 2: 16.8 ms vs 18.1 at the 1M bound). The
// tiles' fixed bound, and the upper limit of the per-vertex prefix pull's (pfx_bound).
constexpr int32_t kPfxH = kHubW * 32;
constexpr int kWideLater = 1024;  // wide split after the first bottom-up level
constexpr int kLeanLevel = 3;     // first pull level (1-based) that may run the lean pass
constexpr uint32_t kNoStop = 0xFFFFFFFFu;  // Loop::stop_level: no limit

struct PlanGraph {
  int64_t n = 0, n_eff = 0, nnz = 0;
  bool rows_sorted = false;
  bool relabelled = false;  // ids in degree order (old2new set)
  bool full_pull = false;   // full_pull_ok(tuning, n), see BitparSolver::full_pull
};
struct PlanOpts {
  int wide_degree = 32, wide_default = 32;  // SolverOptions::wide_degree, kDefaultWideDegree
};
// The level loop's state on entry to the level (BitparSolver::Loop; bu_levels = pull levels of
// the batch before this one), H = pfx_bound of the batch (kPfxH once the level is tiled).
struct PlanLevel {
  uint32_t level = 0, stop_level = kNoStop;
  int bu_levels = 0, nparts = 1;
  bool lazy = false, lean_off = false, keep_rows = false, skipped_any = false, on_chunk = false,
       have_active = false, old_stale = false, fsrc_acc = false, forced = false;
  int64_t ev = 0, ef0 = 0, nact = 0, nactw = 0, na = 0;
  int32_t H = kPfxH;
};

// k_bu_full: the all-zero row n is an int32 vertex index (row n + 1 is scratch), so graphs
// with n > INT32_MAX - 2 keep k_bu_narrow
inline bool full_pull_ok(const Tuning& t, int64_t n) { return t.full && n <= (int64_t)INT32_MAX - 2; }

// This graph and tuning can run a prefix level (sorted rows end their prefix at the first id >= H;
// prepare / prepare_queries / tiles_possible build its tables on this alone, whatever the size)
inline bool prefix_capable(const PlanGraph& g, const Tuning& t) {
  return g.rows_sorted && g.n <= INT32_MAX && t.pfx == 2;
}
// ... and is large enough for it: the prefix level needs the big hub bitmap's graphs
inline bool hub_big_graph(int64_t n) { return n > (int64_t)kHubBig * 32 * 4; }
// filtered levels probe the any-visited bitmap before gathering a neighbour's row: while fewer
// than filter_frac of the edges lead to visited vertices (and always on a lazy batch's first pull)
inline bool filter_by_ev(const PlanGraph& g, const Tuning& t, int64_t ev) {
  return (double)ev < t.filter_frac * (double)g.nnz;
}
// lean first-row pass (k_bu_first) on pull level `bl` (1-based) of a batch, list of nact vertices
inline bool lean_list(const Tuning& t, bool count, bool lean_off, int bl, int64_t nact) {
  return t.lean && !lean_off && !count && bl >= kLeanLevel && nact >= t.lean_min;
}
// the first pull level of a batch, at level 2, of a graph that can run it prefix-wise (tiled, or
// per vertex): filtered, i.e. lazy or still below filter_frac, and so with the LDS hub bitmap
inline bool prefix_level(const PlanGraph& g, const Tuning& t, const PlanLevel& s) {
  return prefix_capable(g, t) && s.bu_levels == 0 && s.level == 2 && hub_big_graph(g.n) &&
         (s.lazy || filter_by_ev(g, t, s.ev));
}
// The first pull level at level 2 with the prefix pull streams static vertex tiles
// (bitpar/tiles.hpp) instead of pulling per vertex from active lists, from tiles_w words on
// (4 words: no sparse codes, every visited hub's row gathered: RMAT-26 / 256 groups ran level 2
// in 9.7 ms tiled vs 7.4 ms per vertex). Pure: the caller ANDs in that the tiles exist
// (pfx_tiles builds them on first use), and only when this holds.
inline bool wants_tiles(const PlanGraph& g, const Tuning& t, int W, bool count,
                        const PlanLevel& s) {
  return !count && W >= 4 && W >= t.tiles_w && t.tiles && prefix_level(g, t, s);
}

// one 768-thread prefix pull block at one word: 80 VGPRs, 6 waves per SIMD, so two blocks per CU
// (the 56-KB hub bitmap each) instead of one 1024-thread block: RMAT-30 / 32 groups level 2 35.9
// -> 32.8 ms, RMAT-26 / 16 groups 3.53 -> 3.36 ms (a next-step column id prefetch measured
// slower: 88 VGPRs)
constexpr int pfx_block(int W) { return W == 1 ? 768 : 1024; }
constexpr int pfx_minw(int W) { return W == 1 ? 6 : 4; }

// the narrow-list pull of a level; the letter is the level record's `kind`
enum class PullKind : char {
  Tiled = 't',   // k_pfx_tiles over static tiles (+ tail push)
  Prefix = 'p',  // per-vertex prefix pull (k_bu_narrow PFX) + tail push
  Hub = 'h',     // filtered k_bu_narrow with the LDS hub bitmap (small or big)
  Lean = 'l',    // k_bu_first + overflow pull
  Full = 'f',    // k_bu_full
  Narrow = 'n',  // plain k_bu_narrow (filtered or not)
};
enum class ChunkSched : char { TwoPass, Prefix, DegreeScan };

struct PullPlan {
  // ---- known before the list build
  bool tiled = false, pfx = false, pfx_lists = false, build_lists = false;
  int wide0 = 0, next_wide = 0;
  // ---- the whole level
  PullKind kind = PullKind::Narrow;
  bool lazy_first = false, filter = false, hub_lds = false, hub_big = false;
  int32_t filter_from = INT32_MAX;  // first id that is probed (0) or INT32_MAX (no probes)
  bool fbm_out = false, pfx_nostamp = false, push_after = false, tail_push = false;
  bool skip_now = false, skip3 = false, take_snapshot = false, probe = false;
  bool codes = false;
  double code_deg = 0;
  bool short1 = false;
  int coop = 1;
  ChunkSched chunks = ChunkSched::DegreeScan;
  // the chunk kernel (LDS hub bitmap where hub_lds): the big bitmap; the prefix-level variant,
  // taken when no codes were built
  bool chunk_hub_big = false, chunk_pfxl = false;
  bool full = false;        // the lean pass's overflow goes through k_bu_full
  int block = 256, minw = 4, hub_w = 0;           // the narrow kernel's launch shape
};

// The part of the plan the list build needs (k_build_active returns nact / nactw, which the rest
// reads). `tiled` = wants_tiles(...) and the tiles exist.
inline void plan_lists(PullPlan& p, const PlanGraph& g, const PlanOpts& o, const Tuning& t, int W,
                       const PlanLevel& s, bool tiled) {
  p.tiled = tiled;
  p.next_wide = std::max(o.wide_degree, kWideLater);
  // The untiled prefix level with a low prefix bound (few sources, see pfx_bound) splits its
  // lists by prefix length (k_build_active): most vertices of degree > wide_few then have short
  // prefixes, which the per-vertex pull handles in a few steps instead of a hub chunk each.
  // RMAT-30 / 32 groups (H ~32K): 53.3 -> 51.2 ms per step (level 2 27.0 -> 23.5, levels 3-4
  // +1.4); RMAT-26 / 16 groups (H ~84K) 4.99 -> 4.92; with H >= ~300K (64+ groups on RMAT-26)
  // 0.4-0.6 ms slower, so only below H = 131072.
  p.pfx = prefix_level(g, t, s);
  p.pfx_lists = !tiled && p.pfx && s.H <= 131072;
  p.build_lists = !s.have_active && !tiled;
  // after the first bottom-up level most vertices exit early: a whole wave per chunk pays
  // off only for much higher degrees, so later lists are split at a higher threshold
  // (wide_few only on big graphs: RMAT-22 / 64 groups ran level 2 in 0.66 ms at 32 or 64 and
  // 0.76-0.83 ms at 128; the narrow pull's long rows then have too few vertices to hide behind)
  // (lists split by prefix length on a graph of >= 2^28 non-isolated vertices: half of it;
  // RMAT-30 / 32 groups 51.1 -> 49.5 ms at 64, 49.8 at 48, 52.6 at 32 prefix entries, while
  // RMAT-26 / 16 groups keeps 128: 4.70 ms, 4.84 at 96, 4.95 at 64)
  const bool few = W <= 4 && t.wide_few > 0 && o.wide_degree == o.wide_default &&
                   g.n_eff >= ((int64_t)1 << 23);
  p.wide0 = s.bu_levels != 0 ? p.next_wide
            : !few           ? o.wide_degree
            : (p.pfx_lists && g.n_eff >= ((int64_t)1 << 28)) ? std::max(1, t.wide_few / 2)
                                                             : t.wide_few;
}

// The whole plan; s.nact / s.nactw are the lists this level pulls (after the build).
inline PullPlan plan_pull(const PlanGraph& g, const PlanOpts& o, const Tuning& t, int W, bool count,
                          const PlanLevel& s, bool tiled) {
  PullPlan p;
  plan_lists(p, g, o, t, W, s, tiled);
  const bool first_bu = s.bu_levels == 0;
  const int bl = s.bu_levels + 1;  // this level, 1-based among the batch's pull levels
  // lazy batch, first pull level: rows of vertices nobody visited yet may be stale, so every
  // gathered row must be one of a visited vertex (always filter), and probes / own rows use a
  // snapshot of the any-visited bitmap (a vertex first visited during the level may be
  // probed before its row is written). From the next pull level on the read buffer holds
  // this level's rows, valid for every vertex a pull can reach (see start_batch).
  p.lazy_first = s.lazy && first_bu;
  p.filter = p.lazy_first || filter_by_ev(g, t, s.ev);
  p.filter_from = p.filter ? 0 : INT32_MAX;
  p.hub_lds = p.filter && g.n > (int64_t)kHubW * 32 * 4;
  p.hub_big = hub_big_graph(g.n);
  // dskip (see done_probe): the lean pass skips the rows of the vertices it finishes; a filtered
  // level never follows it in a batch (ev only grows), and the unfiltered kernels all probe
  // (k_bu_full, k_bu_first, the hub chunks; not the per-vertex pulls of tuning full = 0)
  const bool lean_now = lean_list(t, count, s.lean_off, bl, s.nact) && !p.filter && !tiled && !p.pfx;
  const bool may_skip = !count && t.dskip && g.full_pull && !s.keep_rows;
  p.skip_now = lean_now && may_skip;
  // dskip3: the full pull of an unfiltered, non-lean level (RMAT-26 level 3) skips the rows of
  // the vertices it finishes too, but probes nothing itself while no earlier level skipped (its
  // input rows are all current); the later levels probe as after any skipping level
  p.skip3 = !lean_now && t.dskip3 && may_skip && !p.filter && !tiled && !p.pfx;
  p.take_snapshot = !count && g.full_pull;  // (done_probe: a no-op while no level has skipped)
  p.probe = p.take_snapshot && (p.skip_now || s.skipped_any);
  // sparse row codes for the first bottom-up level after level 1 (see k_build_codes); ids with
  // >= code_deg expected set bits keep row gathers (the tiled level has its own bound)
  p.codes = first_bu && s.level == 2 && t.codes && W >= 8 && s.ef0 > 0 && g.n <= INT32_MAX;
  p.code_deg = tiled ? t.tiles_code_deg : t.code_deg;
  // the untiled prefix level (few words) writes its frontier as a bitmap (fbm_tile_, as the tiled
  // one): the next level pulls and reads no list, a push materialises it (materialize_frontier)
  p.fbm_out = p.pfx && !count && !tiled && s.nact + s.nactw > 0;
  // (see k_push_tail_after; needs the whole level in one tiles launch and vertex part 0 of 1)
  p.push_after = p.pfx && tiled && t.push_after && s.nparts == 1 && !s.on_chunk;
  p.tail_push = p.pfx && !p.push_after;  // k_push_tail before the pulls
  // no stamps for the per-vertex prefix pull at <= 4 words: it reads every vertex's pushed row
  // (8W coalesced bytes) instead of a stamp, and the push stores no stamp per edge
  p.pfx_nostamp = p.pfx && !tiled && W <= 4;
  // short first step (one row) from the third bottom-up level on, or with few words: by
  // then most vertices are covered by their first neighbour (RMAT-26, 1024 groups: level
  // 4 3.1 -> 2.5 ms; level 3 prefers full steps: 6.5 vs 6.7 ms)
  p.short1 = bl >= 3 || W <= 4;
  p.kind = tiled       ? PullKind::Tiled
           : p.pfx     ? PullKind::Prefix
           : p.hub_lds ? PullKind::Hub
           : lean_now  ? PullKind::Lean
           // (unfiltered: no probe code at all, fewer VGPRs, on the levels that load every row)
           : (!count && !p.filter && g.full_pull) ? PullKind::Full
                                                  : PullKind::Narrow;
  // the narrow kernel runs one 1024-thread block per CU anyway (VGPR-bound), so its LDS
  // has room for a 4x larger hub bitmap
  p.block = p.kind == PullKind::Prefix ? pfx_block(W) : p.kind == PullKind::Hub ? 1024 : 256;
  p.minw = p.kind == PullKind::Prefix && !count ? pfx_minw(W) : 4;
  p.hub_w = p.kind == PullKind::Prefix ? kHubW
            : p.kind == PullKind::Hub  ? (p.hub_big ? kHubBig : kHubW)
                                       : 0;
  // early exit across a vertex's chunks (coop) everywhere except on an explosive first
  // bottom-up level (level 2: hardly any row gets covered, and round-robin chunk dealing
  // balances the hubs better). When top-down ran longer (RMAT-30: first pull at level 3, most of
  // every hub's groups already visited) the early exit skips most chunks.
  p.coop = !first_bu || s.level != 2 ? 1 : 0;
  // two passes (see k_chunk_first: first chunks, then the rest of the open vertices), the chunks
  // of the row prefixes with ids < H only, or every chunk from a degree scan
  p.chunks = p.coop && !p.pfx && t.chunk2 ? ChunkSched::TwoPass
             : p.pfx                      ? ChunkSched::Prefix
                                          : ChunkSched::DegreeScan;
  // one chunk block per CU with the 128-KB hub bitmap (ids < 1M) except on the prefix level,
  // whose prefixes end at the small one's bound (two blocks per CU)
  p.chunk_hub_big = p.hub_lds && p.hub_big && !p.pfx;
  // (the prefix level without codes: LDS probes only, the next tile's ids in flight)
  p.chunk_pfxl = p.pfx && p.filter && !p.probe && !p.coop;
  p.full = g.full_pull;
  return p;
}

// Pull levels that bu_batch may run: the third pull level on (lists split at kWideLater, every
// row pulled without probes, no lean pass), active lists of at most bu_max vertices, no forced
// directions (s.forced) and no edge counting (k_count_frontier needs per-level host sizes).
// (fsrc_acc: a push level came last; level_bu first clears the accumulator entries of its
// frontier, which later pulls and the next batch expect all-zero)
inline bool pull_batch_ok(const PlanGraph& g, const Tuning& t, bool count, const PlanLevel& s) {
  if (count || t.bu_max <= 0 || t.batch <= 1 || !s.have_active || s.bu_levels < 2 ||
      s.old_stale || s.fsrc_acc || s.na > t.bu_max || s.forced)
    return false;
  if (filter_by_ev(g, t, s.ev)) return false;
  if (lean_list(t, count, s.lean_off, s.bu_levels + 1, s.nact)) return false;
  return s.stop_level == kNoStop || s.level + 2 <= s.stop_level;
}
// what a level of such a batch launches for both lists (its record's kind)
inline PullKind batch_kind(const PlanGraph& g) {
  return g.full_pull ? PullKind::Full : PullKind::Narrow;
}

// The batches of a query set of K groups: each takes the fewest words (a power of two, at most
// max_words) that hold the groups left, i.e. 64 * w groups but for the last.
struct Batch {
  int w;
  int64_t k0, nb;
};
inline Batch batch_at(int64_t K, int64_t k0, int max_words) {
  int w = 1;
  while (w * 64 < K - k0 && w < max_words) w <<= 1;
  return Batch{w, k0, std::min<int64_t>(K - k0, 64 * w)};
}

}  // namespace bp
}  // namespace msbfs
