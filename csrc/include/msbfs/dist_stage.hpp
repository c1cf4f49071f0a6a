// Host-output distance runs (msbfs_solver_run_dist_host): the pass / row arithmetic of staging a
// K x n distance matrix through a device buffer of a few rows and a pinned chunk. Plain host
// code (no HIP), pinned by csrc/tests/host_selftest.cpp.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

namespace msbfs {

// Rows of the device staging buffer: one solver pass (pass_groups; INT64_MAX for the per-group
// solvers, which take any number of groups per call), at most K, and for the per-group solvers
// at most `budget_bytes` of rows (but always one row).
inline int64_t dist_stage_rows(int64_t pass_groups, int64_t K, int64_t n, int64_t budget_bytes) {
  if (K <= 0) return 0;
  int64_t rows = std::min(pass_groups, K);
  if (pass_groups == INT64_MAX) {
    const int64_t row_bytes = std::max<int64_t>(n, 1) * (int64_t)sizeof(int32_t);
    rows = std::min(rows, std::max<int64_t>(1, budget_bytes / row_bytes));
  }
  return std::max<int64_t>(rows, 1);
}

// Elements [a, b) of a dense rows x n matrix (chunk[0] = element a, row-major, no padding) into
// dst, whose rows are ld >= n elements apart; columns [n, ld) of dst are not touched.
inline void dist_scatter_flat(const int32_t* chunk, int64_t a, int64_t b, int64_t n, int64_t ld,
                              int32_t* dst) {
  if (n <= 0) return;
  while (a < b) {
    const int64_t r = a / n, c = a % n;
    const int64_t len = std::min(b - a, n - c);
    std::memcpy(dst + r * ld + c, chunk, (size_t)len * sizeof(int32_t));
    chunk += len;
    a += len;
  }
}

// One staged pass of a host-output run: the dense nb x n matrix on the device comes down in
// pieces of at most `chunk` elements and goes into dst (row 0 = the pass's first row, rows ld
// elements apart). copy(a, b) must leave elements [a, b) of the device matrix in pin[0, b - a)
// before it returns (a device-to-host copy and its wait); nothing here touches the device.
template <class Copy>
inline void dist_stage_download(Copy&& copy, int64_t nb, int64_t n, int64_t chunk, int64_t ld,
                                const int32_t* pin, int32_t* dst) {
  for (int64_t a = 0; a < nb * n; a += chunk) {
    const int64_t b = std::min(a + chunk, nb * n);
    copy(a, b);
    dist_scatter_flat(pin, a, b, n, ld, dst);
  }
}

}  // namespace msbfs
