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

}  // namespace wh
