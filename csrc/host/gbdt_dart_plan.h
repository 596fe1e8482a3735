// The bin-space tree table of the DART dropout walk (gbdt_dart.hip): a tree's
// admission to the table and its 8-byte nodes, the recovery of split bins
// from the cuts, and the plan that cuts a selection of trees into chunks of
// whole trees that fit the kernel's LDS. Free of HIP and torch: the binding
// compiles it and a CPU-only machine can call it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace wh {

// Nodes of a chunk that k_dart_walk keeps in LDS (8 B each: 32 KiB, 8 full
// depth-8 trees), the trees of a chunk (16 B of staging table each), the
// widest bin row it stages and the depth bound of a walk. With 1024 rows per
// tile the rows take 28 KiB at 28 features (two blocks, 32 waves, per CU) and
// 96 KiB at 96 (one block); 4096 nodes and 1024 rows were the fastest of the
// settings measured at 11M x 28 (profiles/gbdt_dart.txt).
constexpr int kDartLdsNodes = 4096;
constexpr int kDartLdsNodesMax = 16384;  // what a launch takes at most (a plan's own budget)
constexpr int kDartMaxTrees = 256;
constexpr int kDartMaxF = 96;
constexpr int kDartMaxDepth = 64;
inline int gbdt_dart_lds_nodes() { return kDartLdsNodes; }

// One node, 8 B, the packing of k_leaf_walk_lds: an inner node is
// {feat:16 | bin:8 | defl:8, left:16 | right:16} with the children numbered
// within the tree; a leaf is {0xffff, fp32 leaf value}.
struct GbdtDartNode {
  uint32_t w0, w1;
};
static_assert(sizeof(GbdtDartNode) == 8, "a dart node is one 8-byte LDS read");
constexpr uint32_t kDartLeaf = 0xffffu;

// One tree's lists (what models/gbdt_tree.py RegTree holds). bin: the split
// bins where they are known (a tree grown on the current cuts), else empty.
struct GbdtDartTree {
  std::vector<int64_t> feat, bin, left, right, defl;
  std::vector<double> cond, leaf;
};

// The bin of a split `x < cond` under a feature's cuts [lo, hi) of cut_vals:
// the index b with (float)cut_vals[lo + b] == (float)cond exactly (rows binned
// by these cuts then go left iff bin <= b), or -1 when cond is no cut.
inline int64_t gbdt_dart_recover_bin(const std::vector<double>& cut_vals, int64_t lo, int64_t hi,
                                     double cond) {
  const float c = (float)cond;
  const auto b = cut_vals.begin() + lo, e = cut_vals.begin() + hi;
  const auto it = std::lower_bound(b, e, c, [](double v, float x) { return (float)v < x; });
  if (it == e || (float)*it != c) return -1;
  return it - b;
}

// Packs a tree into `out` and returns true iff the table admits it: lists of
// one length, 1 <= nodes <= 65535, every inner node i with i < left, right <
// nodes (node ids grow along a walk, so it ends at a leaf), no walk deeper
// than kDartMaxDepth, every split feature < min(65535, the cuts' feature
// count), every split bin known and < 255. Bins come from t.bin when it is
// given, else from cond by gbdt_dart_recover_bin over cut_off [F + 1].
inline bool gbdt_dart_pack(const GbdtDartTree& t, const std::vector<double>& cut_vals,
                           const std::vector<int64_t>& cut_off, std::vector<GbdtDartNode>* out) {
  out->clear();
  const int64_t nn = (int64_t)t.feat.size();
  const int64_t F = (int64_t)cut_off.size() - 1;
  if (nn < 1 || nn > 65535 || (int64_t)t.left.size() != nn || (int64_t)t.right.size() != nn ||
      (int64_t)t.defl.size() != nn || (int64_t)t.cond.size() != nn ||
      (int64_t)t.leaf.size() != nn || (!t.bin.empty() && (int64_t)t.bin.size() != nn))
    return false;
  std::vector<int32_t> depth(nn, 0);
  out->reserve(nn);
  for (int64_t i = 0; i < nn; ++i) {
    const int64_t f = t.feat[i];
    if (f < 0) {
      const float v = (float)t.leaf[i];
      uint32_t bits;
      std::memcpy(&bits, &v, 4);
      out->push_back({kDartLeaf, bits});
      continue;
    }
    const int64_t l = t.left[i], r = t.right[i];
    if (f >= 65535 || f >= F || l <= i || r <= i || l >= nn || r >= nn ||
        depth[i] >= kDartMaxDepth)
      return out->clear(), false;
    depth[l] = depth[r] = depth[i] + 1;
    const int64_t lo = cut_off[f], hi = cut_off[f + 1];
    if (lo < 0 || hi < lo || hi > (int64_t)cut_vals.size()) return out->clear(), false;
    const int64_t b = t.bin.empty() ? gbdt_dart_recover_bin(cut_vals, lo, hi, t.cond[i]) : t.bin[i];
    if (b < 0 || b >= 255) return out->clear(), false;
    out->push_back({(uint32_t)f | (uint32_t)b << 16 | (uint32_t)(t.defl[i] != 0) << 24,
                    (uint32_t)l | (uint32_t)r << 16});
  }
  return true;
}

// A piece of a selection, in selection order. staged: positions [first,
// first + count) of `sel` are whole trees whose nodes, nnode in all, are
// gathered into LDS at stage_off (one offset per tree, in nodes) and walked
// in one launch. Not staged: one tree (count == 1) that the kernel cannot
// take -- it is not in the table (size <= 0) or larger than the budget -- and
// goes to the caller's fallback.
struct GbdtDartChunk {
  int64_t first, count, nnode;
  bool staged;
  std::vector<int64_t> stage_off;
};

// Cuts the selection `sel` (tree ids into tree_sizes, in the order the leaf
// values are added) into chunks in that order, each tree once: a staged
// chunk takes consecutive selected trees while their nodes fit lds_nodes and
// it has fewer than max_trees; a tree with size <= 0 or > lds_nodes is a
// chunk of its own that is not staged.
inline std::vector<GbdtDartChunk> gbdt_dart_plan(const std::vector<int64_t>& tree_sizes,
                                                 const std::vector<int64_t>& sel,
                                                 int64_t lds_nodes,
                                                 int64_t max_trees = kDartMaxTrees) {
  if (lds_nodes < 1 || max_trees < 1) throw std::invalid_argument("dart plan: empty budget");
  std::vector<GbdtDartChunk> chunks;
  bool open = false;  // the last chunk may still take trees
  for (int64_t j = 0; j < (int64_t)sel.size(); ++j) {
    if (sel[j] < 0 || sel[j] >= (int64_t)tree_sizes.size())
      throw std::invalid_argument("dart plan: a selected tree the model does not have");
    const int64_t sz = tree_sizes[sel[j]];
    if (sz <= 0 || sz > lds_nodes) {
      chunks.push_back({j, 1, std::max<int64_t>(sz, 0), false, {}});
      open = false;
    } else if (open && chunks.back().nnode + sz <= lds_nodes && chunks.back().count < max_trees) {
      auto& c = chunks.back();
      c.stage_off.push_back(c.nnode);
      c.count += 1;
      c.nnode += sz;
    } else {
      chunks.push_back({j, 1, sz, true, {0}});
      open = true;
    }
  }
  return chunks;
}

}  // namespace wh
