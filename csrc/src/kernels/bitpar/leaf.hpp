// Leaf folding of the bit-parallel solver: the degree-1 vertices stay out of the traversal and
// are accounted for through their only neighbour. Plain host code (no HIP): the decision and the
// list builder are pinned without a GPU (tests/test_leaf_fold_cpu.py through the C API,
// csrc/tests/leaf_selftest.cpp under the sanitizers). Kernels: bitpar/leaf_kernels.hpp.
//
// On a degree-relabelled graph (degrees non-increasing in the internal id) the vertices of degree
// 1 are the id range [n_core, n_eff). A leaf v with the single edge {v, p} has dist_g(v) =
// dist_g(p) + 1 for every group g it is not a source of, and nothing is reached through it. So
// the traversal runs on the ids < n_core alone (pushes skip targets >= n_core, the pull lists and
// tiles end at n_core), and with leafw[h] = the number of row entries of h that are >= n_core
//
//   F_g = sum over reached core v of dist_g(v)
//       + sum over reached parents h of leafw[h] * (dist_g(h) + 1)      (k_leaf_weigh, per level)
//       - sum over leaf sources s of g with parent p < n_core of (p is a source of g ? 1 : 2)
//       + sum over leaf sources s of g with neighbour p >= n_core, p not a source of g, of 1
//                                                                        (k_leaf_sources)
//
// The second line is added level by level: a parent that gains the bits nw at level L adds
// (L + 1) * leafw[h] to F_g for every set bit g of nw. The third line takes back what the
// second counted for a leaf that is itself a source (distance 0, not dist(p) + 1); the fourth is
// the other end of a two-vertex component, which has no parent below n_core. A vertex whose
// single row entry is itself lies in the range too: it pushes to nothing and, as its own
// neighbour, is "a source of g", so both corrections leave it alone.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace msbfs {
namespace bp {

// Parents of equal small weight sit together so that a block counts them with the bit-sliced
// group counters and multiplies once at the spill: classes 1 .. kLeafClasses, each padded to a
// multiple of kLeafPad list positions (a multiple of every word count's block tile); heavier
// parents follow unpadded and are counted bit by bit.
constexpr int kLeafClasses = 64;
constexpr int kLeafPad = 256;
// Folding pays by the leaves it takes out of every level and costs a pass over the parents'
// rows per level, so it needs a graph where leaves are a large share. Measured with the
// project's generator (ef 16): RMAT scale 14-22 has 17-23 % leaves among the non-isolated
// vertices; a uniform graph of mean degree 16 has ~2e-6 and a grid none. Auto folds from 1/8.
constexpr int64_t kLeafShareDiv = 8;

// What a run is, as far as folding cares (BitparSolver::batch_impl fills it in)
struct LeafRun {
  int leaf_key = -1;        // tuning key leaf: 0 off, 1 on wherever legal, -1 auto
  bool relabelled = false;  // ids in degree order
  bool rows_sorted = false;
  bool count = false;       // edge counting, distance or parent recording (the COUNT passes)
  int nparts = 1;           // hybrid phases: > 1
  bool limited = false;     // a level limit (hybrid phase A)
};
// legal: the traversal can leave the leaves out and still return F
inline bool leaf_fold_legal(const LeafRun& r, int64_t n_core, int64_t n_eff) {
  return r.relabelled && r.rows_sorted && !r.count && r.nparts == 1 && !r.limited &&
         n_core >= 0 && n_core < n_eff && n_eff <= INT32_MAX;
}
inline bool leaf_fold_on(const LeafRun& r, int64_t n_core, int64_t n_eff) {
  if (r.leaf_key == 0 || !leaf_fold_legal(r, n_core, n_eff)) return false;
  if (r.leaf_key > 0) return true;
  return (n_eff - n_core) * kLeafShareDiv >= n_eff;
}

// first id with degree < min_deg of a CSR whose degrees are non-increasing in the id
inline int64_t first_below_degree(const int64_t* rowptr, int64_t n, int64_t min_deg) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid + 1] - rowptr[mid] < min_deg) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
// leafw[h], h < n_core, of a host CSR with sorted rows: the row's tail of ids >= n_core
inline void leaf_weights_host(const int64_t* rowptr, const int32_t* col, int64_t n_core,
                              int32_t* leafw) {
  for (int64_t h = 0; h < n_core; ++h) {
    const int32_t* b = col + rowptr[h];
    const int32_t* e = col + rowptr[h + 1];
    leafw[h] = (int32_t)(e - std::lower_bound(b, e, (int32_t)std::min<int64_t>(n_core, INT32_MAX)));
  }
}

struct LeafLists {
  int64_t n_core = 0, n_eff = 0;
  int64_t parents = 0;   // vertices with leafw > 0
  int64_t attached = 0;  // sum of leafw (leaves whose neighbour is below n_core)
  int64_t max_w = 0;
  int64_t nsmall = 0;    // padded list positions of the classes 1 .. kLeafClasses
  int64_t nheavy = 0;    // parents heavier than that: positions [nsmall, nsmall + nheavy)
  // per list position: the parent (-1: padding) and its weight (padding: its class's)
  std::vector<int32_t> plist, pw;
  std::vector<int32_t> pidx;  // per id < n_core: its list position, -1 for no parent
  int64_t leaves() const { return n_eff - n_core; }
  int64_t positions() const { return nsmall + nheavy; }
};

// The parent lists from leafw[0 .. n_core): a counting sort by weight class, id order within.
inline LeafLists build_leaf_lists(const int32_t* leafw, int64_t n_core, int64_t n_eff) {
  LeafLists L;
  L.n_core = n_core;
  L.n_eff = n_eff;
  int64_t cnt[kLeafClasses + 2] = {};
  for (int64_t h = 0; h < n_core; ++h) {
    const int64_t w = leafw[h];
    if (w <= 0) continue;
    ++L.parents;
    L.attached += w;
    L.max_w = std::max(L.max_w, w);
    ++cnt[w <= kLeafClasses ? w : kLeafClasses + 1];
  }
  int64_t start[kLeafClasses + 2] = {};
  int64_t pos = 0;
  for (int c = 1; c <= kLeafClasses; ++c) {
    start[c] = pos;
    pos += (cnt[c] + kLeafPad - 1) / kLeafPad * kLeafPad;
  }
  L.nsmall = pos;
  start[kLeafClasses + 1] = pos;
  L.nheavy = cnt[kLeafClasses + 1];
  const size_t np = (size_t)(L.nsmall + L.nheavy);
  L.plist.assign(std::max<size_t>(np, 1), -1);
  L.pw.assign(std::max<size_t>(np, 1), 0);
  for (int c = 1; c <= kLeafClasses; ++c) {
    const int64_t end = c < kLeafClasses ? start[c + 1] : L.nsmall;
    for (int64_t i = start[c]; i < end; ++i) L.pw[(size_t)i] = c;
  }
  L.pidx.assign((size_t)std::max<int64_t>(n_core, 1), -1);
  int64_t fill[kLeafClasses + 2];
  std::copy(start, start + kLeafClasses + 2, fill);
  for (int64_t h = 0; h < n_core; ++h) {
    const int64_t w = leafw[h];
    if (w <= 0) continue;
    const int64_t i = fill[w <= kLeafClasses ? w : kLeafClasses + 1]++;
    L.plist[(size_t)i] = (int32_t)h;
    L.pw[(size_t)i] = (int32_t)w;
    L.pidx[(size_t)h] = (int32_t)i;
  }
  return L;
}

}  // namespace bp
}  // namespace msbfs
