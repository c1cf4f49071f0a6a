// Bit-parallel MS-BFS: the pure bit arithmetic of the level kernels — row slices, the new-bits
// step of a pull / finalize, and the carry-save group counters. No HIP in here: host code
// includes it too (csrc/tests/host_selftest.cpp pins every function with hand-written cases).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (the qualifiers behind MSBFS_HD)
#endif

#include <cstdint>

#include "msbfs/common.hpp"

namespace msbfs {
namespace bp {

// VW consecutive 64-group words of a visited row: one lane's slice
template <int VW>
struct V {
  uint64_t w[VW];
};

template <int VW>
MSBFS_HD V<VW> vzero() {
  V<VW> r;
#pragma unroll
  for (int j = 0; j < VW; ++j) r.w[j] = 0;
  return r;
}

// What a vertex gains at a level, on one lane's slice: r = its visited row, acc = the OR of the
// rows pulled (or bits pushed) into it, am = the alive groups of the batch.
template <int VW>
struct NewBits {
  V<VW> nw;      // new bits: acc among the alive groups the row misses
  V<VW> nv;      // the row after the level
  bool anynew;   // some new bit
  bool notfull;  // an alive group still missing after the level
  bool rnz;      // the row was non-zero before (else this is the vertex's first visit)
};
// the alive groups the row misses
template <int VW>
MSBFS_HD V<VW> missing(const V<VW>& r, const V<VW>& am) {
  V<VW> unv;
#pragma unroll
  for (int j = 0; j < VW; ++j) unv.w[j] = ~r.w[j] & am.w[j];
  return unv;
}
// ... from unv = missing(r, am), which a pull computes before its loop (the coverage test)
template <int VW>
MSBFS_HD NewBits<VW> gained(const V<VW>& r, const V<VW>& acc, const V<VW>& unv) {
  NewBits<VW> o;
  o.anynew = o.notfull = o.rnz = false;
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    o.nw.w[j] = acc.w[j] & unv.w[j];
    o.nv.w[j] = r.w[j] | o.nw.w[j];
    o.anynew |= o.nw.w[j] != 0;
    o.notfull |= (unv.w[j] & ~o.nw.w[j]) != 0;
    o.rnz |= r.w[j] != 0;
  }
  return o;
}
template <int VW>
MSBFS_HD NewBits<VW> new_bits(const V<VW>& r, const V<VW>& acc, const V<VW>& am) {
  return gained(r, acc, missing(r, am));
}

// Register-resident bit-sliced (carry-save) counters: bit b of c[j][d] is bit d of the count of
// group (slot*VW + j)*64 + b. Adding a 64-bit new-bits word costs 2*D branch-free ops, vs one
// LDS atomic per set bit in a divergent loop. Spilled to LDS every < 2^D additions (the spill
// routines: common.hpp).
template <int VW, int DD = 6>
struct BitCounter {
  static constexpr int D = DD;
  uint64_t c[VW][D];
  MSBFS_HD void zero() {
#pragma unroll
    for (int j = 0; j < VW; ++j)
#pragma unroll
      for (int d = 0; d < D; ++d) c[j][d] = 0;
  }
  MSBFS_HD void add(const V<VW>& x) {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      uint64_t carry = x.w[j];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const uint64_t t = c[j][d] & carry;
        c[j][d] ^= carry;
        carry = t;
      }
    }
  }
  // bits of word j with a non-zero count
  MSBFS_HD uint64_t any(int j) const {
    uint64_t a = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) a |= c[j][d];
    return a;
  }
  // count of bit b of word j
  MSBFS_HD uint32_t count(int j, int b) const {
    uint32_t v = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) v |= (uint32_t)((c[j][d] >> b) & 1ull) << d;
    return v;
  }
};

}  // namespace bp
}  // namespace msbfs
