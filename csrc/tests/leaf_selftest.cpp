// Stand-alone self-test of the host code of leaf folding (kernels/bitpar/leaf.hpp), built with
// ASan + UBSan (csrc/Makefile target leaf-asan): the core bound, the leaf weights, the parent
// lists (classes, padding, heavy parents, the id -> position map) and the decision, on
// hand-built degree-ordered graphs, and the folded sum against a plain BFS. No HIP: runs on a
// CPU-only machine.
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <utility>
#include <vector>

#include "../src/kernels/bitpar/leaf.hpp"

using namespace msbfs::bp;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

namespace {
struct Csr {
  int64_t n = 0;
  std::vector<int64_t> rowptr;
  std::vector<int32_t> col;
};

// symmetric CSR with sorted rows, the vertices renumbered by descending degree (stable)
Csr degree_ordered(int64_t n, const std::vector<std::pair<int, int>>& edges) {
  std::vector<std::vector<int32_t>> adj((size_t)n);
  for (auto [u, v] : edges) {
    adj[(size_t)u].push_back(v);
    adj[(size_t)v].push_back(u);
  }
  std::vector<int32_t> order((size_t)n), o2n((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = (int32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return adj[(size_t)a].size() > adj[(size_t)b].size();
  });
  for (int64_t i = 0; i < n; ++i) o2n[(size_t)order[(size_t)i]] = (int32_t)i;
  Csr g;
  g.n = n;
  g.rowptr.assign((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    std::vector<int32_t> row;
    for (int32_t x : adj[(size_t)order[(size_t)i]]) row.push_back(o2n[(size_t)x]);
    std::sort(row.begin(), row.end());
    g.col.insert(g.col.end(), row.begin(), row.end());
    g.rowptr[(size_t)i + 1] = (int64_t)g.col.size();
  }
  return g;
}

std::vector<int32_t> bfs(const Csr& g, const std::vector<int32_t>& src, int64_t limit) {
  std::vector<int32_t> d((size_t)g.n, -1);
  std::queue<int32_t> q;
  for (int32_t s : src)
    if (d[(size_t)s] < 0) {
      d[(size_t)s] = 0;
      q.push(s);
    }
  while (!q.empty()) {
    const int32_t u = q.front();
    q.pop();
    if (u >= limit && d[(size_t)u] > 0) continue;
    for (int64_t j = g.rowptr[(size_t)u]; j < g.rowptr[(size_t)u + 1]; ++j) {
      const int32_t v = g.col[(size_t)j];
      if (v >= limit) continue;  // (the folded traversal pushes to no id >= limit)
      if (d[(size_t)v] < 0) {
        d[(size_t)v] = d[(size_t)u] + 1;
        q.push(v);
      }
    }
  }
  return d;
}

void check_graph(const Csr& g, int64_t want_leaves) {
  const int64_t n_core = first_below_degree(g.rowptr.data(), g.n, 2);
  const int64_t n_eff = first_below_degree(g.rowptr.data(), g.n, 1);
  CHECK(n_eff - n_core == want_leaves);
  for (int64_t v = 0; v < g.n; ++v) {
    const int64_t d = g.rowptr[(size_t)v + 1] - g.rowptr[(size_t)v];
    CHECK((d >= 2) == (v < n_core) && (d == 0) == (v >= n_eff));
  }
  std::vector<int32_t> w((size_t)std::max<int64_t>(n_core, 1), 0);
  leaf_weights_host(g.rowptr.data(), g.col.data(), n_core, w.data());
  const LeafLists L = build_leaf_lists(w.data(), n_core, n_eff);
  CHECK(L.nsmall % kLeafPad == 0);
  CHECK((int64_t)L.plist.size() >= L.positions() && (int64_t)L.pw.size() >= L.positions());
  int64_t parents = 0, attached = 0;
  for (int64_t h = 0; h < n_core; ++h) {
    int64_t c = 0;
    for (int64_t j = g.rowptr[(size_t)h]; j < g.rowptr[(size_t)h + 1]; ++j)
      c += g.col[(size_t)j] >= n_core;
    CHECK(w[(size_t)h] == c);
    const int32_t pi = L.pidx[(size_t)h];
    CHECK((c > 0) == (pi >= 0));
    if (c > 0) {
      ++parents;
      attached += c;
      CHECK(pi < L.positions() && L.plist[(size_t)pi] == h && L.pw[(size_t)pi] == c);
      CHECK((c > kLeafClasses) == (pi >= L.nsmall));
    }
  }
  CHECK(parents == L.parents && attached == L.attached);
  // every kLeafPad run of the padded part has one weight; padding is -1
  int64_t listed = 0;
  for (int64_t i = 0; i < L.positions(); ++i) {
    if (i < L.nsmall) CHECK(L.pw[(size_t)i] == L.pw[(size_t)(i / kLeafPad * kLeafPad)]);
    if (i >= L.nsmall) CHECK(L.plist[(size_t)i] >= 0);
    listed += L.plist[(size_t)i] >= 0;
    if (i > 0 && L.plist[(size_t)i] >= 0 && L.plist[(size_t)i - 1] >= 0 &&
        L.pw[(size_t)i] == L.pw[(size_t)i - 1] && i < L.nsmall)
      CHECK(L.plist[(size_t)i] > L.plist[(size_t)i - 1]);  // id order within a class
  }
  CHECK(listed == L.parents);
  // the folded sum of leaf.hpp against the plain BFS, for a few source sets
  for (int32_t s0 = 0; s0 < g.n; s0 += 3) {
    std::vector<int32_t> src = {s0, (int32_t)((s0 * 7 + 1) % g.n), (int32_t)(g.n - 1 - s0 % 2)};
    const std::vector<int32_t> full = bfs(g, src, g.n), core = bfs(g, src, n_core);
    int64_t F = 0, folded = 0;
    for (int64_t v = 0; v < g.n; ++v) F += full[(size_t)v] > 0 ? full[(size_t)v] : 0;
    for (int64_t v = 0; v < n_core; ++v) {
      if (core[(size_t)v] < 0) continue;
      folded += core[(size_t)v] + (int64_t)w[(size_t)v] * (core[(size_t)v] + 1);
    }
    std::vector<char> seen((size_t)g.n, 0), is_src((size_t)g.n, 0);
    for (int32_t s : src) is_src[(size_t)s] = 1;
    for (int32_t s : src) {
      if (s < n_core || s >= n_eff || seen[(size_t)s]) continue;
      seen[(size_t)s] = 1;
      const int32_t p = g.col[(size_t)g.rowptr[(size_t)s]];
      if (p < n_core) folded -= is_src[(size_t)p] ? 1 : 2;
      else if (!is_src[(size_t)p]) folded += 1;
    }
    CHECK(folded == F);
  }
}
}  // namespace

int main() {
  // the decision
  LeafRun r;
  r.relabelled = r.rows_sorted = true;
  CHECK(leaf_fold_on(r, 75, 100) && leaf_fold_on(r, 875, 1000) && !leaf_fold_on(r, 876, 1000));
  CHECK(!leaf_fold_on(r, 100, 100));
  r.leaf_key = 1;
  CHECK(leaf_fold_on(r, 999, 1000) && !leaf_fold_on(r, 1000, 1000));
  r.leaf_key = 0;
  CHECK(!leaf_fold_on(r, 10, 1000));
  r.leaf_key = 1;
  for (int k = 0; k < 5; ++k) {
    LeafRun x = r;
    if (k == 0) x.relabelled = false;
    if (k == 1) x.rows_sorted = false;
    if (k == 2) x.count = true;
    if (k == 3) x.nparts = 2;
    if (k == 4) x.limited = true;
    CHECK(!leaf_fold_on(x, 10, 1000));
  }
  CHECK(!leaf_fold_on(r, 10, (int64_t)INT32_MAX + 1));

  // a hub with 300 leaves (a heavy parent), a path, two-vertex components, a doubled edge, a
  // self-loop (two row entries), isolated vertices
  {
    std::vector<std::pair<int, int>> e;
    for (int i = 0; i < 300; ++i) e.push_back({0, 10 + i});
    for (int i = 1; i < 6; ++i) e.push_back({i - 1, i});
    e.push_back({5, 6});       // 6: the path's end, a leaf
    e.push_back({7, 8});       // a two-vertex component
    e.push_back({9, 0});
    e.push_back({9, 0});       // doubled edge: degree 2
    e.push_back({320, 320});   // self-loop
    for (int i = 0; i < 70; ++i) e.push_back({3, 330 + i});  // weight 70 > kLeafClasses
    for (int i = 0; i < 5; ++i) e.push_back({4, 410 + i});
    check_graph(degree_ordered(420, e), 300 + 1 + 2 + 70 + 5);
  }
  // a star: the centre's whole row is leaves
  {
    std::vector<std::pair<int, int>> e;
    for (int i = 1; i < 700; ++i) e.push_back({0, i});
    check_graph(degree_ordered(700, e), 699);
  }
  // a 6 x 7 grid: no leaves, nothing listed
  {
    std::vector<std::pair<int, int>> e;
    for (int r0 = 0; r0 < 6; ++r0)
      for (int c = 0; c < 7; ++c) {
        if (c + 1 < 7) e.push_back({r0 * 7 + c, r0 * 7 + c + 1});
        if (r0 + 1 < 6) e.push_back({r0 * 7 + c, (r0 + 1) * 7 + c});
      }
    check_graph(degree_ordered(42, e), 0);
  }
  // no vertices, no edges
  check_graph(degree_ordered(0, {}), 0);
  check_graph(degree_ordered(5, {}), 0);
  // many parents of each small weight: the classes' padding
  {
    std::vector<std::pair<int, int>> e;
    int v = 600;
    for (int h = 0; h < 600; ++h) {
      e.push_back({h, (h + 1) % 600});
      for (int k = 0; k < h % 5; ++k) e.push_back({h, v++});
    }
    check_graph(degree_ordered(v, e), v - 600);
  }
  printf("leaf selftest: ok\n");
  return 0;
}
