// CPU multi-source BFS: BASELINE config 1 ("serial CPU BFS on 1 rank") and the test oracle.
// Semantics follow GPUMultiSourceBFS + ComputeFofU (main.cu:40-89): all valid sources of a group
// start at distance 0, out-of-range sources are ignored, F sums the finite distances only.
#include <algorithm>
#include <atomic>
#include <thread>

#include "msbfs/graph.hpp"

namespace msbfs {

int64_t cpu_msbfs_F(const HostCsr& g, const int32_t* src, int64_t nsrc, std::vector<int32_t>& dist,
                    std::vector<int64_t>& queue, int64_t* edges, int32_t* levels) {
  const int64_t n = g.n;
  dist.assign(n, -1);
  queue.resize(std::max<int64_t>(n, 1));
  int64_t head = 0, tail = 0;
  for (int64_t i = 0; i < nsrc; ++i) {
    const int64_t s = src[i];
    if (s >= 0 && s < n && dist[s] < 0) {
      dist[s] = 0;
      queue[tail++] = s;
    }
  }
  int64_t F = 0, deg_sum = 0;
  int32_t maxd = 0;
  while (head < tail) {
    const int64_t u = queue[head++];
    const int32_t du = dist[u];
    F += du;
    maxd = std::max(maxd, du);
    const int64_t b = g.rowptr[u], e = g.rowptr[u + 1];
    deg_sum += e - b;
    for (int64_t j = b; j < e; ++j) {
      const int32_t v = g.col[j];
      if (dist[v] < 0) {
        dist[v] = du + 1;
        queue[tail++] = v;
      }
    }
  }
  if (edges) *edges = deg_sum / 2;
  if (levels) *levels = tail ? maxd + 1 : 0;
  return F;
}

void cpu_parent_row(const HostCsr& g, const int32_t* dist, int32_t* parent) {
  for (int64_t v = 0; v < g.n; ++v) {
    const int32_t d = dist[v];
    int32_t p = d == 0 ? (int32_t)v : -1;
    if (d > 0) {
      for (int64_t j = g.rowptr[v], e = g.rowptr[v + 1]; j < e; ++j) {
        if (dist[g.col[j]] == d - 1) {
          p = g.col[j];
          break;
        }
      }
    }
    parent[v] = p;
  }
}

void cpu_profile_row(const int32_t* dist, int64_t n, int64_t k, const RunOutputs& p) {
  int64_t* h = p.hist ? p.hist + k * p.hist_ld : nullptr;
  if (h) std::fill(h, h + p.nbins, int64_t{0});
  int64_t reach = 0;
  int32_t mx = -1;
  for (int64_t v = 0; v < n; ++v) {
    const int32_t d = dist[v];
    if (d < 0) continue;
    ++reach;
    mx = std::max(mx, d);
    if (h) ++h[std::min<int64_t>(d, p.nbins - 1)];
  }
  if (p.reach) p.reach[k] = reach;
  if (p.ecc) p.ecc[k] = mx;
}

void cpu_msbfs_all(const HostCsr& g, const QuerySet& q, std::vector<int64_t>& F,
                   std::vector<int64_t>* edges, int nthreads, const RunOutputs& out) {
  const int64_t K = q.K();
  F.assign(K, 0);
  if (edges) edges->assign(K, 0);
  if (nthreads <= 0) nthreads = default_threads();
  nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, K));
  std::atomic<int64_t> next{0};
  auto worker = [&] {
    std::vector<int32_t> dist;
    std::vector<int64_t> queue;
    for (;;) {
      const int64_t k = next.fetch_add(1);
      if (k >= K) break;
      int64_t e = 0;
      F[k] = cpu_msbfs_F(g, q.ids.data() + q.off[k], q.off[k + 1] - q.off[k], dist, queue, &e);
      if (edges) (*edges)[k] = e;
      // (the worker's distance array already is the row: -1 unreached, 0 the valid sources)
      if (out.dist) std::copy(dist.begin(), dist.begin() + g.n, out.dist + k * out.ld);
      if (out.parent) cpu_parent_row(g, dist.data(), out.parent + k * out.ld);
      if (out.asked == RunOutputs::kProfile) cpu_profile_row(dist.data(), g.n, k, out);
    }
  };
  if (nthreads == 1) {
    worker();
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; ++t) th.emplace_back(worker);
  for (auto& t : th) t.join();
}

}  // namespace msbfs
