// The task plan of the GBDT ranking kernels (csrc/hip/gbdt_rank.hip): the
// query groups of a matrix, given as row offsets, checked and sorted into the
// three classes of work the kernels take. Free of HIP and torch: the binding
// compiles it and a CPU-only machine can call it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace wh {

// Rows of a group that one wavefront takes (one row per lane).
constexpr int kRankWaveRows = 64;

// Rows of a group that a block keeps resident in LDS. Per row the kernels
// hold {margin, label, 1 / partner count, rank discount}: 4 x 4 B = 16 B, so
// 4096 rows are 64 KiB of the CU's 160 KiB and two such blocks fit a CU. A
// launch sizes its LDS by its own largest group, so smaller groups leave room
// for more blocks. Measured (benchmarks/bench_gbdt_rank.py, profiles/
// gbdt_rank.txt): one group of 1024 / 2048 / 4096 rows resident against the
// same group streamed in tiles of half its rows differ by less than 1 %
// (182.1 / 180.5, 346.9 / 345.8, 676.9 / 675.3 us): the kernels are bound by
// the pairs' arithmetic, not by LDS traffic, so the capacity does not set the
// speed. 4096 stays: the largest size that still leaves two blocks per CU,
// and a group up to it costs each block one tile load and one barrier pair.
constexpr int kRankLdsRows = 4096;
inline int gbdt_rank_lds_rows() { return kRankLdsRows; }

// Group ids per class, larger groups first (ties: lower id first):
//   small  1 .. kRankWaveRows rows   one wavefront per group
//   block  .. lds_rows rows          a block per 256 rows, the group resident in LDS
//   tiled  above lds_rows            a block per 256 rows, partners streamed in tiles
struct GbdtRankPlan {
  std::vector<int32_t> small, block, tiled;
  int64_t max_block_rows = 0, max_tiled_rows = 0;  // the largest group of a list (0: none)
};

// group_off [count] = Q + 1 offsets into n rows: the first 0, non-decreasing,
// the last n. Throws std::invalid_argument otherwise, for no offsets at all
// and for n above INT32_MAX. Empty groups are in no list.
inline GbdtRankPlan gbdt_rank_plan(const int64_t* group_off, size_t count, int64_t n,
                                   int64_t lds_rows = kRankLdsRows) {
  if (count == 0) throw std::invalid_argument("group offsets are empty");
  if (n < 0 || n > INT32_MAX) throw std::invalid_argument("ranking rows must fit int32");
  if (count - 1 > (size_t)INT32_MAX) throw std::invalid_argument("too many groups");
  if (lds_rows < kRankWaveRows) throw std::invalid_argument("lds_rows below a wavefront's rows");
  if (group_off[0] != 0) throw std::invalid_argument("group offsets must start at 0");
  for (size_t q = 1; q < count; ++q)
    if (group_off[q] < group_off[q - 1])
      throw std::invalid_argument("group offsets decrease at group " + std::to_string(q - 1));
  if (group_off[count - 1] != n)
    throw std::invalid_argument("group offsets end at " + std::to_string(group_off[count - 1]) +
                                ", the matrix has " + std::to_string(n) + " rows");
  GbdtRankPlan p;
  for (size_t q = 0; q + 1 < count; ++q) {
    const int64_t len = group_off[q + 1] - group_off[q];
    if (len == 0) continue;
    (len <= kRankWaveRows ? p.small : len <= lds_rows ? p.block : p.tiled).push_back((int32_t)q);
  }
  const auto larger_first = [&](int32_t a, int32_t b) {
    return group_off[a + 1] - group_off[a] > group_off[b + 1] - group_off[b];
  };
  for (auto* v : {&p.small, &p.block, &p.tiled}) std::stable_sort(v->begin(), v->end(), larger_first);
  if (!p.block.empty()) p.max_block_rows = group_off[p.block[0] + 1] - group_off[p.block[0]];
  if (!p.tiled.empty()) p.max_tiled_rows = group_off[p.tiled[0] + 1] - group_off[p.tiled[0]];
  return p;
}

}  // namespace wh
