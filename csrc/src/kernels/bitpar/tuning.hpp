// Algorithm tuning of the bit-parallel solver: the struct, its "key=value" parser and the
// process-wide default (MSBFS_TUNE). Plain host code: the pull-level plan (pull_plan.hpp) and
// the host self test use it without the HIP headers.
#pragma once

#include <cstdint>
#include <string>

namespace msbfs {
namespace bp {

// Algorithm tuning of the bit-parallel solver. Defaults are the measured best (RMAT-26 / 1024
// groups, RMAT-30, road grid, uniform graphs; see README). Set per solver through
// Solver::tune ("key=value,key=value"; msbfs_solver_tune in the C API, Solver(tuning=...) in
// Python) or process-wide through the one variable MSBFS_TUNE (same syntax; echoed on stderr).
// Unknown keys and malformed values are errors, never ignored. Every key is exercised by a GPU
// oracle test (tests/test_gpu_kernels.py).
struct Tuning {
  // push -> pull once the frontier's degree sum exceeds gamma x n_eff (0: off). Level 2, where
  // the prefix pull applies, uses gamma2 (< 0: gamma): RMAT-30 / 16 groups 296 -> 106 ms
  double gamma = 1.0, gamma2 = 0.25;
  bool gamma2_auto = true;  // gamma2 not set explicitly: only skewed graphs use it (gamma_for)
  // first bottom-up level: 0 = whole-row pull; 2 = prefix pull (ids < 458752, the 56-KB LDS hub
  // bitmap) + tail push (RMAT-26 level 2: 16.8 ms vs 21.2 for whole rows)
  int pfx = 2;
  // sparse single-group row codes on the first bottom-up level; ids with degree >=
  // code_deg * nnz / (source degree sum), i.e. >= code_deg expected set bits, keep row gathers
  int codes = 1;
  double code_deg = 3.0;
  // lean first-row pass on the third and later pull levels (k_bu_first) for active lists of at
  // least lean_min vertices (RMAT-26 level 4: 2.48 -> 2.07 ms)
  int lean = 1;
  int64_t lean_min = 1 << 20;
  int lazy = 1;        // no per-batch fill of the visited buffer (see start_batch)
  int td_fused = 1;    // device-driven batches run the one-kernel k_td_fused levels
  // k_td_fused walks the frontier bitmap from this frontier size on (road grid 4896^2, two
  // sessions: 64 groups 306.8-307.2 -> 302.9-304.3 ms, 16 groups 142.8 -> 139.4, 256 groups
  // 1377 -> 1370 against 65536; 32768 ran 310, 262144 305 ms at 64 groups)
  int64_t td_bm = 131072;
  int batch = 64;      // top-down levels per device-driven batch (1 = host-driven levels)
  // pull levels from the third on run as device-driven batches (bu_batch) while the active lists
  // hold at most bu_max vertices (0 = host-driven pull levels; needs batch > 1)
  int64_t bu_max = 1 << 20;
  int tiles = 1;       // first pull level over static vertex tiles (bitpar/tiles.hpp)
  int tiles_w = 8;     // fewest words per vertex that take the tiled first pull level (4, 8 or 16)
  // unfiltered pull levels (the second pull level on, lean overflow, device-driven batches) run
  // k_bu_full (structured-buffer rows, wave-private list queues; bitpar/pull_full.hpp) instead
  // of k_bu_narrow
  int full = 1;
  // done rows are never read (k_bu_full): pulls probe a level-start snapshot of the done bitmap
  // instead of gathering done neighbours' rows, and the rows of vertices finishing on an
  // unfiltered pull level are not written (a push level right after gets them restored)
  int dskip = 1;
  // tiled first pull level: the tail push after the tiles, into the output rows (one GPU, no
  // chunked exchange; k_push_tail_after) instead of into acc rows every tile vertex reads
  // (RMAT-26 / 1024 groups: level 2 12.5 -> 10.95 ms, 20.7-21.3 -> 19.1-19.8 ms per step)
  int push_after = 1;
  // dskip on the non-lean unfiltered full pulls too (RMAT-26 level 3: 5.80 -> 5.68 ms, 1 GB of
  // row stores fewer; see level_bu)
  int dskip3 = 1;
  // two-pass chunk scheduling of the wide vertices on early-exit levels (k_chunk_first):
  // RMAT-26 / 1024 groups level 3 5.70 -> 5.30 ms
  int chunk2 = 1;
  // wide threshold of the first pull level for passes of <= 4 words (no tiles there) while
  // SolverOptions::wide_degree is at its default, on graphs of >= 2^23 non-isolated vertices:
  // RMAT-26, level 2, 128 groups 6.54 -> 6.01 ms, 256 groups 7.49 -> 7.11 ms (32 -> 128; 512 and
  // 2048 slower; RMAT-22 prefers 32-64). 0: wide_degree as given
  int wide_few = 128;
  // prefix bound of the untiled first pull level (ids below it are pulled, the frontier vertices
  // at or above it push; <= 458752, the LDS hub bitmap's bound). 0: from the batch's source
  // count (BitparSolver::pfx_bound)
  int pfx_h = 0;
  // pull levels probe the any-visited bitmap before a neighbour's row while fewer than this
  // fraction of the edges lead to visited vertices (ev < filter_frac * nnz)
  double filter_frac = 0.5;
  // code_deg of the tiled level: codes are cheap there (a 4-byte load and LDS ORs instead of a
  // row gather), so rows with up to ~12 expected bits are worth a try (RMAT-26 level 2: 3 ->
  // 12: 13.85 -> 13.32 ms)
  double tiles_code_deg = 12.0;
  // leaf folding (bitpar/leaf.hpp): the degree-1 vertices of a degree-relabelled graph stay out
  // of a plain F run's traversal and are counted through their parents. 0 off, 1 on wherever it
  // is legal, -1 (default) on where leaves are at least 1/8 of the non-isolated vertices
  int leaf = -1;
  // test key: at most this many blocks (1..2048) for every grid-stride level kernel, the tiled
  // first pull level's k_pfx_tiles (one block per CU otherwise) included, so that one block of a
  // small graph runs the hundreds of tiles at which the register counters spill and the LDS
  // queues flush mid-loop (tests/test_block_loops_gpu.py, tests/test_prefix_level_gpu.py).
  // 0 (default): no cap, every grid as computed. Changes no decision and no count, only how many
  // blocks share a level
  int max_grid = 0;
  std::string dirs;    // forced per-level directions 'T'/'B' (tests, experiments)

  void set(const std::string& key, const std::string& value);
  void parse(const std::string& spec);  // "k=v,k=v" (or ";")
  static const Tuning& process_default();  // defaults + MSBFS_TUNE, read once per process
};

}  // namespace bp
}  // namespace msbfs
