// The per-level host tables of the GBDT host grower (csrc/bind/gbdt_ops.cc
// gbdt_grow): the tiling of the row positions by the live node segments and
// the word offsets of the level's one upload. Free of HIP and torch: the
// binding and the host self-test compile the same code.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

namespace wh {

// The live segments {begin, end, node} (disjoint, any order) tile [0, n):
// returns {begin, node} in position order with node = -1 for every gap (rows
// of finished leaves) in front of, between and behind them. The same rule as
// models/gbdt.py _pos_node; gbdt.hip k_seg_fill / k_part_cursor expand it.
inline std::vector<std::array<int, 2>> gbdt_level_tiles(std::vector<std::array<int, 3>> segs,
                                                          int64_t n) {
  std::sort(segs.begin(), segs.end());
  std::vector<std::array<int, 2>> tiles;
  int cur = 0;
  for (auto& a : segs) {
    if (a[0] > cur) tiles.push_back({cur, -1});
    tiles.push_back({a[0], a[2]});
    cur = a[1];
  }
  if (cur < n) tiles.push_back({cur, -1});
  return tiles;
}

// The host grower's one upload per level, as int32 word offsets (the same in
// the pinned staging copy and on the device): node feat / bin / seg_beg /
// seg_end [nnode], defl (bytes, rounded up to words) [nnode], tiles beg /
// node [nt], split table [nsplit x 4], parent slots [nsplit], the
// partition's left / right cursors [nnode] (device-updated)
struct GbdtNodeTables {
  int64_t feat, bin, sb, se, defl, tb, tn, sp, par, lc, rc, nwords;
  GbdtNodeTables(int64_t nnode, int64_t nt, int64_t nsplit)
      : feat(0), bin(nnode), sb(2 * nnode), se(3 * nnode), defl(4 * nnode),
        tb(defl + (nnode + 3) / 4), tn(tb + nt), sp(tn + nt), par(sp + 4 * nsplit),
        lc(par + nsplit), rc(lc + nnode), nwords(rc + nnode) {}
};

// monotone_constraints: a node's weight interval {lo, hi}. A weight is
// clamped to it; an accepted split on a feature of sign c cuts it at the mean
// of the children's clamped weights (wl, wr): c > 0 gives the left child
// {lo, mid} and the right {mid, hi}, c < 0 the mirror image, c == 0 hands the
// interval down unchanged. The same rule as models/gbdt.py child_bounds and
// gbdt.hip k_gd_apply.
using GbdtBounds = std::array<double, 2>;

inline double gbdt_clamp_weight(double w, const GbdtBounds& b) {
  return w < b[0] ? b[0] : (w > b[1] ? b[1] : w);
}

inline std::array<GbdtBounds, 2> gbdt_child_bounds(int c, const GbdtBounds& b, double wl,
                                                   double wr) {
  const double mid = (wl + wr) / 2;
  if (c > 0) return {GbdtBounds{b[0], mid}, GbdtBounds{mid, b[1]}};
  if (c < 0) return {GbdtBounds{mid, b[1]}, GbdtBounds{b[0], mid}};
  return {b, b};
}

// interaction_constraints on one 64-bit word: bit i < 63 of a feature's mask
// says that group i contains it, and a feature in no group holds bit 63 alone.
// A node's state is the set of groups that contain every feature split on
// above it: all ones at the root, which therefore admits every feature; a
// node admits feature f iff state & mask[f] != 0. The children of a split on
// f narrow the state by mask[f] and drop bit 63, so nothing is admitted below
// a split on an ungrouped feature. The same rule as models/gbdt_objective.py
// interaction_child and gbdt.hip k_gd_apply.
constexpr uint64_t kGbdtInterFree = 1ull << 63;
constexpr uint64_t kGbdtInterRoot = ~0ull;

inline uint64_t gbdt_child_state(uint64_t state, uint64_t fmask) {
  return state & fmask & ~kGbdtInterFree;
}

}  // namespace wh
