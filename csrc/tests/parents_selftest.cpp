// Stand-alone self-test of the host code behind the BFS parent output, built with ASan + UBSan and
// with TSan (csrc/Makefile targets parents-asan / parents-tsan): cpu_parent_row, the threaded
// cpu_msbfs_all with a parent matrix (what msbfs_cpu_run_parents runs), and the row arithmetic
// msbfs_solver_run_parents_host stages its two matrices with (dist_stage_rows on half the byte
// budget, dist_stage_download per matrix). No HIP: runs on a CPU-only machine.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msbfs/dist_stage.hpp"
#include "msbfs/graph.hpp"

using namespace msbfs;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

namespace {
constexpr int32_t kSentinel = 123456789;

// the contract, checked entry by entry against an independent distance array
void check_rows(const HostCsr& g, const QuerySet& q, int64_t k, const int32_t* dist,
                const int32_t* parent) {
  std::vector<int32_t> d;
  std::vector<int64_t> queue;
  cpu_msbfs_F(g, q.ids.data() + q.off[k], q.off[k + 1] - q.off[k], d, queue);
  for (int64_t v = 0; v < g.n; ++v) {
    CHECK(dist[v] == d[v]);
    if (d[v] < 0) {
      CHECK(parent[v] == -1);
    } else if (d[v] == 0) {
      CHECK(parent[v] == (int32_t)v);
    } else {
      // the FIRST row entry one level nearer, whichever vertex discovered v
      int32_t first = -1;
      for (int64_t j = g.rowptr[v]; j < g.rowptr[v + 1] && first < 0; ++j)
        if (d[g.col[j]] == d[v] - 1) first = g.col[j];
      CHECK(first >= 0 && parent[v] == first);
    }
  }
}

void run_case(const HostCsr& g, const QuerySet& q, int nthreads, int64_t pad) {
  const int64_t K = q.K(), ld = g.n + pad;
  std::vector<int32_t> dist((size_t)(K * ld + 1), kSentinel), parent((size_t)(K * ld + 1), kSentinel);
  std::vector<int64_t> F, F2;
  cpu_msbfs_all(g, q, F, nullptr, nthreads, RunOutputs::parents(dist.data(), parent.data(), ld));
  cpu_msbfs_all(g, q, F2, nullptr, 1);
  CHECK(F == F2);
  for (int64_t k = 0; k < K; ++k) {
    check_rows(g, q, k, dist.data() + k * ld, parent.data() + k * ld);
    for (int64_t c = g.n; c < ld; ++c)
      CHECK(dist[k * ld + c] == kSentinel && parent[k * ld + c] == kSentinel);
  }
  CHECK(dist[K * ld] == kSentinel && parent[K * ld] == kSentinel);
  // a parent matrix alone is not a mode: the distance matrix may be left out, the parents not
  // computed from anything else
  std::vector<int32_t> p2((size_t)(K * ld + 1), kSentinel);
  cpu_msbfs_all(g, q, F2, nullptr, nthreads, RunOutputs::parents(nullptr, p2.data(), ld));
  CHECK(p2 == parent);
}

// a parent that the queue's discoverer rule gets wrong: 0 - 1, 0 - 2, 3's row is {2, 1}
void discoverer_case() {
  EdgeList el;
  el.n = 5;  // (vertex 4 isolated)
  el.u = {0, 0, 2, 1};
  el.v = {1, 2, 3, 3};
  const HostCsr g = build_csr(el, 1, true);
  QuerySet q;
  q.add({0});
  std::vector<int32_t> dist(5), parent(5);
  std::vector<int64_t> F;
  cpu_msbfs_all(g, q, F, nullptr, 1, RunOutputs::parents(dist.data(), parent.data(), 5));
  CHECK(g.col[g.rowptr[3]] == 2);  // 3's first row entry is 2; BFS from 0 discovers 3 from 1
  CHECK(parent[3] == 2 && parent[1] == 0 && parent[2] == 0 && parent[0] == 0 && parent[4] == -1);
  CHECK(dist[3] == 2 && dist[4] == -1 && F[0] == 4);
}

// the staging of msbfs_solver_run_parents_host on host memory: two "device" matrices of `rows`
// rows, each brought down through dist_stage_download (the loop capi.cpp runs, with a memcpy as
// its copy step) into a padded host matrix
void staging_case(int64_t pass_groups, int64_t K, int64_t n, int64_t budget, int64_t chunk,
                  int64_t pad) {
  const int64_t ld = n + pad;
  const int64_t rows = dist_stage_rows(pass_groups, K, n, budget / 2);
  CHECK(rows >= 1 && rows <= std::max<int64_t>(K, 1));
  if (pass_groups == INT64_MAX && rows > 1) CHECK(2 * rows * n * 4 <= budget);
  std::vector<int32_t> host[2], dev[2], pin((size_t)chunk);
  for (int m = 0; m < 2; ++m) {
    host[m].assign((size_t)(K * ld), kSentinel);
    dev[m].assign((size_t)(rows * std::max<int64_t>(n, 1)), 0);
  }
  for (int64_t k0 = 0; k0 < K; k0 += rows) {
    const int64_t nb = std::min(rows, K - k0);
    for (int m = 0; m < 2; ++m)
      for (int64_t i = 0; i < nb * n; ++i) dev[m][i] = (int32_t)((k0 + i / n) * 1000 + i % n + m);
    for (int m = 0; m < 2; ++m)
      dist_stage_download(
          [&](int64_t a, int64_t b) {
            CHECK(0 <= a && a < b && b - a <= chunk && b <= nb * n);
            std::copy(dev[m].begin() + a, dev[m].begin() + b, pin.begin());
          },
          nb, n, chunk, ld, pin.data(), host[m].data() + k0 * ld);
  }
  for (int m = 0; m < 2; ++m)
    for (int64_t k = 0; k < K; ++k)
      for (int64_t c = 0; c < ld; ++c)
        CHECK(host[m][k * ld + c] == (c < n ? (int32_t)(k * 1000 + c + m) : kSentinel));
}
}  // namespace

int main() {
  discoverer_case();
  {
    const HostCsr g = build_csr(gen_uniform(2000, 1500, 4), 2);  // (many small components)
    QuerySet q = gen_queries(g.n, 11, 3, 5);
    q.add({});
    q.add({-1, (int32_t)g.n, 2147483647});
    q.add({7, 7, 7, (int32_t)g.n - 1, 0});
    for (int t : {1, 3, 8}) run_case(g, q, t, t == 3 ? 7 : 0);
  }
  {
    const HostCsr g = build_csr(gen_rmat(9, 8, 3), 2);  // (hubs, duplicate edges, self-loops)
    run_case(g, gen_queries(g.n, 9, 2, 6), 4, 5);
  }
  {
    const HostCsr g = build_csr(gen_grid(12, 17, 0.9, 3, 2), 1);
    run_case(g, gen_queries(g.n, 5, 2, 4), 2, 0);
  }
  staging_case(128, 300, 37, int64_t{256} << 20, 1000, 7);   // bit-parallel: passes of 128 rows
  staging_case(INT64_MAX, 9, 50, 1200, 64, 3);                 // per-group: 3 rows per matrix
  staging_case(INT64_MAX, 5, 50, 100, 7, 0);                   // budget below one row: one row
  staging_case(INT64_MAX, 4, 0, 1 << 20, 16, 2);               // n = 0
  printf("parents selftest: ok\n");
  return 0;
}
