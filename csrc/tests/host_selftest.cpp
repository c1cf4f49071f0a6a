// Host-code self test for the sanitizer builds (make -C csrc asan / tsan).
//
// The reference has no race detection or sanitizer story at all (its kernel relies on a benign
// data race, main.cu:16-38). GPU AddressSanitizer is not available on the target
// pool, so the sanitizers cover the native HOST code: the multi-threaded generators, the parallel
// CSR build (count -> scan -> scatter over threads), the mmap loaders / writers and the CSR
// sidecar cache, the query-parallel CPU BFS, the in-process thread collectives of the
// single-process multi-GPU mode, and the bit-parallel solver's plain host code: the tuning parser,
// the batch split of a query set and the plan of a pull level (a table of hand-written cases).
// Every parallel result is compared with a single-thread run, so a data race that changes a
// value fails the test even without TSan.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <unistd.h>

#include "../cli/thread_group.hpp"
#include "../src/kernels/bitpar/bits.hpp"
#include "../src/kernels/bitpar/pull_plan.hpp"
#include "msbfs/dist_stage.hpp"
#include "msbfs/graph.hpp"

using namespace msbfs;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                     \
    }                                                              \
  } while (0)

// The in-process communicator of the single-process multi-GPU mode (cli/thread_group.hpp): P
// threads run many rounds of every collective back to back (the slots and the barrier are
// reused immediately, the case a missing barrier would corrupt) and check every result.
static void thread_group_selftest() {
  const int P = 5, rounds = 300;
  ThreadGroup g(P);
  std::vector<int> bad(P, 0);
  std::vector<std::thread> th;
  for (int r = 0; r < P; ++r)
    th.emplace_back([&, r] {
      for (int it = 0; it < rounds; ++it) {
        int64_t buf[3] = {r == it % P ? (int64_t)it : -1, r == it % P ? (int64_t)(it * 7) : -1, 0};
        tg_bcast(g, r, buf, 2 * sizeof(int64_t), it % P);
        bad[r] += buf[0] != it || buf[1] != it * 7;
        bad[r] += tg_allreduce_min(g, r, (uint64_t)(1000 + r * 13 + it)) != (uint64_t)(1000 + it);
        bad[r] += tg_allreduce_max(g, r, (double)(r + it)) != (double)(P - 1 + it);
        int64_t v[4] = {r, 1, it, -r};
        tg_allreduce_sum(g, r, v, 4);
        bad[r] += v[0] != P * (P - 1) / 2 || v[1] != P || v[2] != (int64_t)P * it ||
                  v[3] != -P * (P - 1) / 2;
        std::vector<uint64_t> all;
        tg_allgather(g, r, (uint64_t)(r * r + it), all);
        for (int k = 0; k < P; ++k) bad[r] += all[k] != (uint64_t)(k * k + it);
        // all-to-all: rank r sends (j + 1 + it % 3) words of value r*100 + j to rank j
        std::vector<int64_t> sc(P), rc(P);
        std::vector<uint64_t> send, recv;
        for (int j = 0; j < P; ++j) {
          sc[j] = j + 1 + it % 3;
          rc[j] = r + 1 + it % 3;
          for (int64_t w = 0; w < sc[j]; ++w) send.push_back((uint64_t)(r * 100 + j));
        }
        recv.assign(P * (r + 1 + it % 3), ~0ull);
        tg_alltoallv(g, r, send.data(), sc, recv.data(), rc);
        for (int j = 0, o = 0; j < P; ++j)
          for (int64_t w = 0; w < rc[j]; ++w) bad[r] += recv[o++] != (uint64_t)(j * 100 + r);
      }
    });
  for (auto& t : th) t.join();
  for (int r = 0; r < P; ++r) CHECK(bad[r] == 0);
}

// ---- the pull-level plan (kernels/bitpar/pull_plan.hpp): which kernels a bottom-up level of the
// bit-parallel solver launches. Every expectation below is written out by hand from level_bu's
// predicates as they stood before the plan existed.
namespace plan_test {
using namespace msbfs::bp;

struct Case {
  PlanGraph g;
  PlanOpts o;
  Tuning t;
  int W = 16;
  bool count = false;
  PlanLevel s;
  bool tiles_built = true;  // pfx_tiles would hand out a tile set
};
// what level_bu does with a case: tiles only when wanted and there, H = the tiles' bound then
static PullPlan plan(Case c) {
  c.g.full_pull = full_pull_ok(c.t, c.g.n);
  const bool tiled = wants_tiles(c.g, c.t, c.W, c.count, c.s) && c.tiles_built;
  if (tiled) c.s.H = kPfxH;
  return plan_pull(c.g, c.o, c.t, c.W, c.count, c.s, tiled);
}
static bool batch_ok(Case c) {
  c.g.full_pull = full_pull_ok(c.t, c.g.n);
  return pull_batch_ok(c.g, c.t, c.count, c.s);
}
static Case with(Case c, const char* spec) {
  c.t.parse(spec);
  return c;
}
// names of the plan fields in which a and b differ, "a b c"
static std::string diff(const PullPlan& a, const PullPlan& b) {
  std::string d;
#define F(x) \
  if (!(a.x == b.x)) d += std::string(d.empty() ? "" : " ") + #x;
  F(tiled) F(pfx) F(pfx_lists) F(build_lists) F(wide0) F(next_wide) F(kind) F(lazy_first)
  F(filter) F(hub_lds) F(hub_big) F(filter_from) F(fbm_out) F(pfx_nostamp) F(push_after)
  F(tail_push) F(skip_now) F(skip3) F(take_snapshot) F(probe) F(codes) F(code_deg) F(short1)
  F(coop) F(chunks) F(chunk_hub_big) F(chunk_pfxl) F(full) F(block) F(minw) F(hub_w)
#undef F
  return d;
}
static char kind(const PullPlan& p) { return (char)p.kind; }

// RMAT-26-like: relabelled, sorted rows, a lazy batch of W words at pull level `bu` (0-based)
static Case rmat26(int W, uint32_t level, int bu) {
  Case c;
  c.g.n = (int64_t)1 << 26;
  c.g.n_eff = 33000000;
  c.g.nnz = (int64_t)1 << 31;
  c.g.rows_sorted = c.g.relabelled = true;
  c.W = W;
  c.s.level = level;
  c.s.bu_levels = bu;
  c.s.lazy = true;
  c.s.have_active = bu > 0;
  c.s.ef0 = 1000000;
  c.s.ev = bu == 0 ? 5000000 : (int64_t)6 << 28;  // (0.6 nnz from the second pull on)
  c.s.nact = bu == 0 ? 30000000 : bu == 1 ? 20000000 : 2000000;
  c.s.nactw = 100000;
  c.s.na = c.s.nact + c.s.nactw;
  c.s.skipped_any = bu >= 2;  // (level 3 skipped rows: dskip3)
  c.s.H = kPfxH;              // (pfx_bound of >= 128 groups on this graph)
  return c;
}
// a graph of n vertices, mean degree 16, first pull of a lazy batch at `level`
static Case sized(int64_t n, uint32_t level) {
  Case c = rmat26(16, level, 0);
  c.g.n = c.g.n_eff = n;
  c.g.nnz = 16 * n;
  c.s.ev = n / 8;
  c.s.nact = n / 2;
  return c;
}

static void cases() {
  const int kNone = INT32_MAX;
  {  // level 2, 16 words, tiles there
    const PullPlan p = plan(rmat26(16, 2, 0));
    CHECK(kind(p) == 't' && p.tiled && p.pfx && !p.pfx_lists && !p.build_lists);
    CHECK(p.push_after && !p.tail_push && !p.fbm_out && !p.pfx_nostamp);
    CHECK(p.codes && p.code_deg == 12.0);
    CHECK(p.lazy_first && p.filter && p.filter_from == 0 && p.hub_lds && p.hub_big);
    CHECK(p.coop == 0 && !p.skip_now && !p.skip3 && p.take_snapshot && !p.probe);
  }
  Case untiled = rmat26(16, 2, 0);
  untiled.tiles_built = false;
  {  // the same level, tiles not there: the per-vertex prefix pull
    const PullPlan p = plan(untiled);
    CHECK(kind(p) == 'p' && !p.tiled && p.pfx && p.build_lists && p.wide0 == 32);
    CHECK(p.block == 1024 && p.minw == 4 && p.hub_w == 14336);
    CHECK(!p.pfx_nostamp && p.fbm_out && p.tail_push && !p.push_after);
    CHECK(p.codes && p.code_deg == 3.0 && p.coop == 0 && p.chunks == ChunkSched::Prefix);
    CHECK(!p.chunk_hub_big && p.chunk_pfxl);
    CHECK(!p.pfx_lists);  // H = 458752
    Case c = untiled;
    c.s.H = 131072;
    CHECK(diff(plan(c), p) == "pfx_lists");
    c.s.H = 131073;
    CHECK(diff(plan(c), p) == "");
  }
  {  // level 3, the second pull, unfiltered
    const PullPlan p = plan(rmat26(16, 3, 1));
    CHECK(kind(p) == 'f' && !p.short1 && p.skip3 && !p.skip_now && p.take_snapshot && !p.probe);
    CHECK(!p.filter && p.filter_from == kNone && !p.lazy_first && !p.hub_lds && !p.pfx);
    CHECK(p.coop == 1 && p.chunks == ChunkSched::TwoPass && !p.chunk_hub_big && !p.codes);
    CHECK(!p.build_lists && p.next_wide == 1024 && !p.fbm_out && !p.tail_push);
    CHECK(!batch_ok(rmat26(16, 3, 1)));  // (the third pull level on)
  }
  {  // level 4, a long list: the lean pass
    const PullPlan p = plan(rmat26(16, 4, 2));
    CHECK(kind(p) == 'l' && p.skip_now && !p.skip3 && p.probe && p.full && p.short1);
    CHECK(!batch_ok(rmat26(16, 4, 2)));
  }
  {  // level 4, a short list: the full pull with the one-row first step; may run in a batch
    Case c = rmat26(16, 4, 2);
    c.s.nact = 500000;
    c.s.na = 600000;
    const PullPlan p = plan(c);
    CHECK(kind(p) == 'f' && p.short1 && p.skip3 && !p.skip_now && p.probe);
    CHECK(batch_ok(c) && (char)batch_kind(c.g) == 'n');  // (full_pull not filled in: narrow)
    c.g.full_pull = true;
    CHECK((char)batch_kind(c.g) == 'f');
    c.s.na = ((int64_t)1 << 20) + 1;  // > bu_max
    CHECK(!batch_ok(c));
    c.s.na = 600000;
    c.s.fsrc_acc = true;
    CHECK(!batch_ok(c));
    c.s.fsrc_acc = false;
    c.s.forced = true;
    CHECK(!batch_ok(c));
    c.s.forced = false;
    c.s.stop_level = 5;  // level 4 done, 5 the last: no room for two
    CHECK(!batch_ok(c));
    c.s.stop_level = 6;
    CHECK(batch_ok(c));
  }
  // the edge-counting pass (never lazy): no tiles, no lean, no full pull, no fused counting
  // (hence no frontier bitmap), no skipping and no done snapshot
  for (int bu = 0; bu < 3; ++bu)
    for (int64_t nact : {(int64_t)500000, (int64_t)20000000}) {
      Case c = rmat26(16, 2 + bu, bu);
      c.count = true;
      c.s.lazy = false;
      c.s.nact = nact;
      c.s.na = nact + c.s.nactw;
      const PullPlan p = plan(c);
      CHECK(kind(p) == (bu == 0 ? 'p' : 'n') && !p.tiled && !p.fbm_out && p.minw == 4);
      CHECK(!p.skip_now && !p.skip3 && !p.take_snapshot && !p.probe);
      CHECK(!batch_ok(c));
    }
  {  // 2 words: no tiles, lists split at wide_few, no stamps
    const PullPlan p = plan(rmat26(2, 2, 0));
    CHECK(kind(p) == 'p' && p.wide0 == 128 && p.pfx_nostamp && p.block == 1024 && p.minw == 4);
    CHECK(!p.codes && p.fbm_out && p.tail_push);
    Case c = rmat26(2, 2, 0);
    c.o.wide_degree = 48;  // (not the default: as given)
    CHECK(plan(c).wide0 == 48);
  }
  {  // 1 word: two 768-thread blocks per CU
    Case c = rmat26(1, 2, 0);
    c.s.H = 80000;
    const PullPlan p = plan(c);
    CHECK(kind(p) == 'p' && p.block == 768 && p.minw == 6 && p.pfx_lists && p.wide0 == 128);
  }
  {  // >= 2^28 non-isolated vertices with lists split by prefix length: half of wide_few
    Case c = rmat26(1, 2, 0);
    c.g.n = (int64_t)1 << 30;
    c.g.n_eff = (int64_t)1 << 29;
    c.g.nnz = (int64_t)1 << 35;
    c.s.H = 32768;
    CHECK(plan(c).pfx_lists && plan(c).wide0 == 64);
    c.s.H = kPfxH;
    CHECK(!plan(c).pfx_lists && plan(c).wide0 == 128);
  }
  {  // hybrid phase A: tiled, the tail push before the tiles, no skipping
    Case c = rmat26(16, 2, 0);
    c.s.keep_rows = c.s.on_chunk = true;
    c.s.nparts = 8;
    CHECK(diff(plan(c), plan(rmat26(16, 2, 0))) == "push_after tail_push");
    CHECK(kind(plan(c)) == 't' && !plan(c).push_after && !plan(c).skip_now && !plan(c).skip3);
    c.s.level = 3;
    c.s.bu_levels = 1;
    c.s.ev = (int64_t)6 << 28;
    CHECK(kind(plan(c)) == 'f' && !plan(c).skip3);  // (keep_rows)
  }
  {  // the first pull at level 3: no prefix level, early exit across chunks
    const PullPlan p = plan(rmat26(16, 3, 0));
    CHECK(kind(p) == 'h' && !p.pfx && !p.tiled && p.coop == 1 && p.hub_w == 32768);
    CHECK(p.block == 1024 && p.filter && p.lazy_first && !p.codes && !p.tail_push && !p.fbm_out);
    CHECK(p.chunks == ChunkSched::TwoPass && p.chunk_hub_big && !p.chunk_pfxl && p.build_lists);
  }
  {  // sizes that separate the LDS-hub variants
    const int64_t big = (int64_t)1 << 22, small = 14336 * 128;
    CHECK(kind(plan(sized(big + 1, 2))) == 't' && plan(sized(big + 1, 2)).pfx);
    CHECK(kind(plan(sized(big + 1, 3))) == 'h' && plan(sized(big + 1, 3)).hub_w == 32768);
    for (uint32_t level : {2u, 3u}) {
      PullPlan p = plan(sized(big, level));
      CHECK(kind(p) == 'h' && p.hub_w == 14336 && !p.pfx && !p.tiled && !p.hub_big);
      CHECK(p.hub_lds && !p.chunk_hub_big && !p.chunk_pfxl);
      p = plan(sized(small + 1, level));
      CHECK(kind(p) == 'h' && p.hub_w == 14336 && p.block == 1024);
      p = plan(sized(small, level));
      CHECK(kind(p) == 'n' && p.filter && !p.hub_lds && p.hub_w == 0 && p.block == 256);
    }
    CHECK(prefix_capable(sized(small, 2).g, Tuning()));  // (prepare's tables: whatever the size)
    Case c = sized(big + 1, 2);
    c.g.rows_sorted = false;
    CHECK(!prefix_capable(c.g, c.t) && kind(plan(c)) == 'h');
  }
  // tuning switches: the key flips what it names (and what follows from it), nothing else
  const Case l2 = rmat26(16, 2, 0), l3 = rmat26(16, 3, 1), l4 = rmat26(16, 4, 2);
  CHECK(diff(plan(with(untiled, "pfx=0")), plan(untiled)) ==
        "pfx kind fbm_out tail_push chunks chunk_hub_big chunk_pfxl hub_w");
  CHECK(kind(plan(with(l2, "pfx=0"))) == 'h' && !plan(with(l2, "pfx=0")).tiled);
  CHECK(diff(plan(with(l2, "tiles=0")), plan(untiled)) == "");
  CHECK(kind(plan(rmat26(4, 2, 0))) == 'p');
  CHECK(kind(plan(with(rmat26(4, 2, 0), "tiles_w=4"))) == 't');
  CHECK(kind(plan(with(rmat26(2, 2, 0), "tiles_w=4"))) == 'p');
  CHECK(diff(plan(with(l2, "codes=0")), plan(l2)) == "codes");
  CHECK(diff(plan(with(l4, "lean=0")), plan(l4)) == "kind skip_now skip3");
  CHECK(kind(plan(with(l4, "lean=0"))) == 'f');
  CHECK(diff(plan(with(l4, "lean_min=2000001")), plan(with(l4, "lean=0"))) == "");
  CHECK(diff(plan(with(l3, "full=0")), plan(l3)) == "kind skip3 take_snapshot full");
  CHECK(kind(plan(with(l3, "full=0"))) == 'n');
  {
    Case c = l4;
    c.s.skipped_any = false;
    CHECK(diff(plan(with(c, "dskip=0")), plan(c)) == "skip_now probe");
    CHECK(diff(plan(with(l3, "dskip=0")), plan(l3)) == "skip3");
  }
  CHECK(diff(plan(with(l3, "dskip3=0")), plan(l3)) == "skip3");
  CHECK(diff(plan(with(l3, "chunk2=0")), plan(l3)) == "chunks");
  CHECK(plan(with(l3, "chunk2=0")).chunks == ChunkSched::DegreeScan);
  CHECK(diff(plan(with(l2, "push_after=0")), plan(l2)) == "push_after tail_push");
  {
    const PullPlan p = plan(with(l3, "filter_frac=2"));  // every pull level filtered
    CHECK(kind(p) == 'h' && p.filter && p.filter_from == 0 && p.hub_w == 32768 && !p.skip3);
    CHECK(!batch_ok(with(l4, "filter_frac=2")));
    Case c = l3;
    c.s.ev = (int64_t)1 << 28;  // 0.125 nnz: filtered by default
    CHECK(kind(plan(c)) == 'h' && kind(plan(with(c, "filter_frac=0"))) == 'f');
    CHECK(plan(with(l2, "filter_frac=0")).filter);  // (the lazy first pull always filters)
  }
}

static void batches() {
  struct B {
    int w;
    int64_t k0, nb;
  };
  auto walk = [](int64_t K, int mw) {
    std::vector<B> v;
    for (Batch b = batch_at(K, 0, mw); b.k0 < K; b = batch_at(K, b.k0 + b.nb, mw))
      v.push_back(B{b.w, b.k0, b.nb});
    return v;
  };
  auto same = [](const std::vector<B>& a, const std::vector<B>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
      if (a[i].w != b[i].w || a[i].k0 != b[i].k0 || a[i].nb != b[i].nb) return false;
    return true;
  };
  CHECK(walk(0, 16).empty());
  CHECK(same(walk(1, 16), {{1, 0, 1}}));
  CHECK(same(walk(64, 16), {{1, 0, 64}}));
  CHECK(same(walk(65, 16), {{2, 0, 65}}));
  CHECK(same(walk(130, 16), {{4, 0, 130}}));
  CHECK(same(walk(1024, 16), {{16, 0, 1024}}));
  CHECK(same(walk(1500, 16), {{16, 0, 1024}, {8, 1024, 476}}));
  CHECK(same(walk(1, 2), {{1, 0, 1}}));
  CHECK(same(walk(64, 2), {{1, 0, 64}}));
  CHECK(same(walk(65, 2), {{2, 0, 65}}));
  CHECK(same(walk(130, 2), {{2, 0, 128}, {1, 128, 2}}));
  CHECK(same(walk(1024, 2), {{2, 0, 128}, {2, 128, 128}, {2, 256, 128}, {2, 384, 128},
                             {2, 512, 128}, {2, 640, 128}, {2, 768, 128}, {2, 896, 128}}));
  CHECK(same(walk(1500, 2), {{2, 0, 128}, {2, 128, 128}, {2, 256, 128}, {2, 384, 128},
                             {2, 512, 128}, {2, 640, 128}, {2, 768, 128}, {2, 896, 128},
                             {2, 1024, 128}, {2, 1152, 128}, {2, 1280, 128}, {2, 1408, 92}}));
}

static void tuning() {
  Tuning t;
  t.parse("pfx=0,lean_min=5;tiles_w=16,filter_frac=0.25,dirs=TB.T");
  CHECK(t.pfx == 0 && t.lean_min == 5 && t.tiles_w == 16 && t.filter_frac == 0.25);
  CHECK(t.dirs == "TB.T" && t.lean == 1 && t.bu_max == (1 << 20));  // (the rest: defaults)
  auto fails_with = [](const char* spec, const char* what) {
    try {
      Tuning().parse(spec);
    } catch (const msbfs::Error& e) {
      return std::string(e.what()).find(what) != std::string::npos;
    }
    return false;
  };
  CHECK(fails_with("nosuch=1", "unknown key 'nosuch'"));
  CHECK(fails_with("lean=abc", "bad value 'abc' for lean"));
  CHECK(fails_with("lean=", "bad value"));
  CHECK(fails_with("lean", "expected key=value"));
  CHECK(fails_with("pfx=1", "pfx must be"));
  // the test key max_grid: 0 (default, no cap) or a block count of 1..2048
  CHECK(Tuning().max_grid == 0 && t.max_grid == 0);
  for (const int g : {0, 1, 3, 2048}) {
    Tuning m;
    m.parse("max_grid=" + std::to_string(g));
    CHECK(m.max_grid == g);
  }
  CHECK(fails_with("max_grid=-1", "max_grid must be"));
  CHECK(fails_with("max_grid=4096", "max_grid must be"));
  CHECK(fails_with("max_grid=2049", "max_grid must be"));
  CHECK(fails_with("max_grid=1.5", "max_grid must be"));
  CHECK(fails_with("nosuch=1", "max_grid"));  // (the unknown-key message lists it)
}
}  // namespace plan_test

// ---- the kernels' pure bit helpers (bitpar/bits.hpp), on hand-written cases
namespace bits_test {
using namespace msbfs::bp;

static void new_bits_cases() {
  const uint64_t ALL = ~0ull;
  {  // empty row: everything pulled among the alive groups is new, and it is a first visit
    const V<1> r{{0}}, acc{{0x0F0Full}}, am{{0x00FFull}};
    const NewBits<1> o = new_bits(r, acc, am);
    CHECK(o.nw.w[0] == 0x000Full && o.nv.w[0] == 0x000Full);
    CHECK(o.anynew && o.notfull && !o.rnz);  // (alive groups 4-7 still missing)
    const NewBits<1> none = new_bits(r, V<1>{{0}}, am);
    CHECK(none.nw.w[0] == 0 && none.nv.w[0] == 0 && !none.anynew && none.notfull && !none.rnz);
  }
  {  // full row: nothing new, nothing missing, whatever was pulled
    const V<1> r{{ALL}}, acc{{0x1234ull}}, am{{ALL}};
    const NewBits<1> o = new_bits(r, acc, am);
    CHECK(o.nw.w[0] == 0 && o.nv.w[0] == ALL && !o.anynew && !o.notfull && o.rnz);
    // full on the alive groups only: the same, and the row keeps its dead groups' bits
    const NewBits<1> p = new_bits(V<1>{{0xFF0Full}}, V<1>{{0x00F0ull}}, V<1>{{0x000Full}});
    CHECK(p.nw.w[0] == 0 && p.nv.w[0] == 0xFF0Full && !p.anynew && !p.notfull && p.rnz);
  }
  {  // acc outside am: bits of groups that are not alive are dropped
    const V<1> r{{0x1ull}}, acc{{0xF0ull}}, am{{0x0Full}};
    const NewBits<1> o = new_bits(r, acc, am);
    CHECK(o.nw.w[0] == 0 && o.nv.w[0] == 0x1ull && !o.anynew && o.notfull && o.rnz);
    const NewBits<1> q = new_bits(r, V<1>{{0xF6ull}}, am);  // (bits 1, 2 inside)
    CHECK(q.nw.w[0] == 0x6ull && q.nv.w[0] == 0x7ull && q.anynew && q.notfull && q.rnz);
    const NewBits<1> f = new_bits(r, V<1>{{0xFEull}}, am);  // (completes the alive groups)
    CHECK(f.nw.w[0] == 0xEull && f.nv.w[0] == 0xFull && f.anynew && !f.notfull);
  }
  {  // one word of two: the flags OR over the words, the words stay apart
    const V<2> r{{0, 0x3ull}}, acc{{0, 0xCull}}, am{{0x1ull, 0xFull}};
    const NewBits<2> o = new_bits(r, acc, am);
    CHECK(o.nw.w[0] == 0 && o.nw.w[1] == 0xCull && o.nv.w[0] == 0 && o.nv.w[1] == 0xFull);
    CHECK(o.anynew && o.notfull && o.rnz);  // (word 0 misses its one alive group)
    const NewBits<2> p = new_bits(r, V<2>{{0x1ull, 0xCull}}, am);
    CHECK(p.nw.w[0] == 0x1ull && p.nw.w[1] == 0xCull && p.anynew && !p.notfull && p.rnz);
    const NewBits<2> z = new_bits(V<2>{{0, 0}}, V<2>{{0, 0x8ull}}, am);
    CHECK(z.nw.w[1] == 0x8ull && z.anynew && z.notfull && !z.rnz);
    // gained() on the precomputed missing groups is the same function
    const V<2> unv = missing(r, am);
    CHECK(unv.w[0] == 0x1ull && unv.w[1] == 0xCull);
    const NewBits<2> g = gained(r, acc, unv);
    CHECK(g.nw.w[1] == o.nw.w[1] && g.nv.w[1] == o.nv.w[1] && g.notfull == o.notfull);
  }
}

// after 2^D - 1 adds of random words every count equals the number of adds with that bit set
template <int D>
static void bit_counter_case(uint64_t seed) {
  constexpr int VW = 2, N = (1 << D) - 1;
  BitCounter<VW, D> bc;
  bc.zero();
  uint32_t want[VW][64] = {};
  for (int i = 0; i < N; ++i) {
    V<VW> x;
    for (int j = 0; j < VW; ++j) {
      x.w[j] = msbfs::mix64(seed + (uint64_t)(i * VW + j));
      if (i % 7 == 3) x.w[j] = ~0ull;  // (some full words: the carries run through every slice)
      for (int b = 0; b < 64; ++b) want[j][b] += (uint32_t)((x.w[j] >> b) & 1ull);
    }
    bc.add(x);
  }
  bool ok = true, any_ok = true;
  for (int j = 0; j < VW; ++j) {
    uint64_t nz = 0;
    for (int b = 0; b < 64; ++b) {
      ok &= bc.count(j, b) == want[j][b];
      if (want[j][b]) nz |= 1ull << b;
    }
    any_ok &= bc.any(j) == nz;
  }
  CHECK(ok);
  CHECK(any_ok);
  bc.zero();
  CHECK(bc.any(0) == 0 && bc.any(1) == 0 && bc.count(1, 63) == 0);
}

static void bit_counter_cases() {
  bit_counter_case<5>(11);
  bit_counter_case<6>(12);
  bit_counter_case<7>(13);
  // every add with all bits set: the count saturates the D slices exactly at 2^D - 1
  BitCounter<1, 5> bc;
  bc.zero();
  for (int i = 0; i < 31; ++i) bc.add(V<1>{{~0ull}});
  CHECK(bc.count(0, 0) == 31 && bc.count(0, 63) == 31);
}
}  // namespace bits_test

// the pass / row arithmetic of the host-output distance runs (msbfs/dist_stage.hpp)
static void dist_stage_cases() {
  // bit-parallel: one pass of rows, never more than K; no budget applies
  CHECK(dist_stage_rows(1024, 5000, 1 << 20, 1 << 20) == 1024);
  CHECK(dist_stage_rows(128, 100, 1 << 20, 1) == 100);
  CHECK(dist_stage_rows(64, 0, 10, 1 << 20) == 0);
  // per-group solvers: any number of groups per call, rows bounded by the budget, at least one
  CHECK(dist_stage_rows(INT64_MAX, 9, 1000, 4000 * 4) == 4);
  CHECK(dist_stage_rows(INT64_MAX, 3, 1000, 4000 * 4) == 3);
  CHECK(dist_stage_rows(INT64_MAX, 9, 1000, 10) == 1);
  CHECK(dist_stage_rows(INT64_MAX, 9, 0, 10) == 2);  // (n = 0 counts as one element)
  // flat chunks of a 3 x 5 matrix into rows 8 apart: every chunking gives the same rows and
  // leaves the padding alone
  const int64_t n = 5, ld = 8, rows = 3;
  std::vector<int32_t> src(rows * n);
  for (int64_t i = 0; i < rows * n; ++i) src[i] = (int32_t)(100 + i);
  for (int64_t chunk : {1, 2, 4, 5, 7, 15, 40}) {
    std::vector<int32_t> dst(rows * ld, -7);
    for (int64_t a = 0; a < rows * n; a += chunk) {
      const int64_t b = std::min(a + chunk, rows * n);
      dist_scatter_flat(src.data() + a, a, b, n, ld, dst.data());
    }
    bool ok = true;
    for (int64_t r = 0; r < rows; ++r)
      for (int64_t c = 0; c < ld; ++c) ok &= dst[r * ld + c] == (c < n ? 100 + r * n + c : -7);
    CHECK(ok);
  }
  std::vector<int32_t> none(4, -7);
  dist_scatter_flat(src.data(), 0, 0, n, ld, none.data());
  dist_scatter_flat(src.data(), 0, 3, 0, ld, none.data());  // (n = 0: nothing to place)
  CHECK(none == std::vector<int32_t>(4, -7));
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string gp = dir + "/selftest_g.bin", qp = dir + "/selftest_q.bin";
  const int T = 8;
  thread_group_selftest();
  plan_test::cases();
  plan_test::batches();
  plan_test::tuning();
  bits_test::new_bits_cases();
  bits_test::bit_counter_cases();
  dist_stage_cases();
  // generators: threaded == serial
  EdgeList e1 = gen_rmat(12, 8, 5, 0.57, 0.19, 0.19, true, 1);
  EdgeList e8 = gen_rmat(12, 8, 5, 0.57, 0.19, 0.19, true, T);
  CHECK(e1.u == e8.u && e1.v == e8.v);
  EdgeList u1 = gen_uniform(3000, 20000, 9, 1), u8 = gen_uniform(3000, 20000, 9, T);
  CHECK(u1.u == u8.u && u1.v == u8.v);
  // CSR build: threaded (stable order) == serial
  HostCsr c1 = build_csr(e1, 1, true), c8 = build_csr(e1, T, true);
  CHECK(c1.rowptr == c8.rowptr && c1.col == c8.col);
  CHECK(c1.nnz() == 2 * e1.m());
  // file round trip + sidecar cache (written on the first load, read on the second)
  write_edge_list_bin(gp, e1);
  EdgeList r = read_edge_list_bin(gp);
  CHECK(r.n == e1.n && r.u == e1.u && r.v == e1.v);
  unlink((gp + ".csr").c_str());
  HostCsr l1 = load_graph(gp, true, T);
  HostCsr l2 = load_graph(gp, true, T);
  CHECK(l1.rowptr == c1.rowptr && l2.rowptr == c1.rowptr && l2.col == l1.col);
  // queries: legacy and extended formats
  QuerySet q = gen_queries(c1.n, 300, 5, 7);
  write_query_bin(qp, q, false);  // K > 255 -> extended
  QuerySet q2 = read_query_bin(qp);
  CHECK(q2.off == q.off && q2.ids == q.ids);
  // query-parallel CPU BFS: threaded == serial, F and traversed edges
  std::vector<int64_t> F1, F8, E1, E8;
  cpu_msbfs_all(l1, q, F1, &E1, 1);
  cpu_msbfs_all(l1, q, F8, &E8, T);
  CHECK(F1 == F8 && E1 == E8);
  CHECK(argmin_first(F1) >= 0);
  // ... and its distance rows: threaded == serial, padding untouched, each row sums to its F
  {
    const int64_t ld = l1.n + 3, K = q.K();
    std::vector<int32_t> d1((size_t)(K * ld), 77), d8((size_t)(K * ld), 77);
    std::vector<int64_t> Fd1, Fd8;
    cpu_msbfs_all(l1, q, Fd1, nullptr, 1, RunOutputs::distances(d1.data(), ld));
    cpu_msbfs_all(l1, q, Fd8, nullptr, T, RunOutputs::distances(d8.data(), ld));
    CHECK(Fd1 == F1 && Fd8 == F1 && d1 == d8);
    bool ok = true;
    for (int64_t k = 0; k < K; ++k) {
      int64_t sum = 0;
      for (int64_t v = 0; v < l1.n; ++v) sum += std::max(d1[k * ld + v], 0);
      ok &= sum == F1[k];
      for (int64_t v = l1.n; v < ld; ++v) ok &= d1[k * ld + v] == 77;
    }
    CHECK(ok);
    // ... and its level profiles (what msbfs_cpu_run_profile runs): threaded == serial == the
    // distance rows' counts, the tail folded into the last of 3 columns, padding untouched
    const int64_t nb = 3, pld = 5;
    std::vector<int64_t> r1((size_t)K), r8((size_t)K), h1((size_t)(K * pld), -5), h8 = h1, Fp1, Fp8;
    std::vector<int32_t> e1v((size_t)K), e8v((size_t)K);
    const RunOutputs p1 = RunOutputs::profile(r1.data(), e1v.data(), h1.data(), nb, pld);
    const RunOutputs p8 = RunOutputs::profile(r8.data(), e8v.data(), h8.data(), nb, pld);
    cpu_msbfs_all(l1, q, Fp1, nullptr, 1, p1);
    cpu_msbfs_all(l1, q, Fp8, nullptr, T, p8);
    CHECK(Fp1 == F1 && Fp8 == F1 && r1 == r8 && e1v == e8v && h1 == h8);
    ok = true;
    for (int64_t k = 0; k < K; ++k) {
      int64_t cnt[3] = {0, 0, 0}, reach = 0;
      int32_t mx = -1;
      for (int64_t v = 0; v < l1.n; ++v) {
        const int32_t d = d1[k * ld + v];
        if (d < 0) continue;
        ++reach;
        mx = std::max(mx, d);
        ++cnt[std::min<int32_t>(d, 2)];
      }
      ok &= reach == r1[k] && mx == e1v[k];
      for (int b = 0; b < 3; ++b) ok &= h1[k * pld + b] == cnt[b];
      for (int64_t b = nb; b < pld; ++b) ok &= h1[k * pld + b] == -5;
    }
    CHECK(ok);
  }
  unlink(gp.c_str());
  unlink((gp + ".csr").c_str());
  unlink(qp.c_str());
  printf("host selftest: %s (%d failed checks)\n", fails ? "FAILED" : "ok", fails);
  return fails ? 1 : 0;
}
