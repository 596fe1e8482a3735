// The packed forest of the GBDT forest prediction (gbdt_forest.hip): the
// trees of a model flattened into one node table, checked so that a walk
// provably ends, and the plan that cuts the table into chunks of whole trees
// that fit the kernel's LDS. Free of HIP and torch: the binding compiles it
// and a CPU-only machine can call it.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace wh {

// Nodes of a chunk that the forest kernels keep in LDS: 8192 x 16 B = 128 KiB
// of the CU's 160 KiB (one block per CU; 16 full depth-8 trees per chunk).
constexpr int kForestLdsNodes = 8192;
inline int gbdt_forest_lds_nodes() { return kForestLdsNodes; }

// One node, 16 B (one ds_read_b128): an inner node is {feat << 1 | defl,
// threshold, left, right} with the children numbered within the tree; a leaf
// is {-1, leaf value, 0, 0}.
struct GbdtForestNode {
  int32_t fd;
  float v;
  int32_t left, right;
};
static_assert(sizeof(GbdtForestNode) == 16, "a forest node is one 16-byte LDS read");

// The trees' lists (what models/gbdt_tree.py RegTree holds), one entry per tree.
struct GbdtForestTrees {
  std::vector<std::vector<int64_t>> feat, left, right, defl;
  std::vector<std::vector<double>> cond, leaf;
};

// Flattens the trees into `nodes` and `tree_off` [T + 1]. Every inner node i
// of a tree of nn nodes must have i < left < nn and i < right < nn (a leaf is
// feat < 0): node ids then grow strictly along any walk, so it ends at a leaf
// after fewer than nn steps and never leaves its tree. A tree that fails
// this, has no node, lists of different lengths or a feature id that does not
// fit throws std::invalid_argument("malformed tree t").
inline void gbdt_forest_pack(const GbdtForestTrees& tr, std::vector<GbdtForestNode>* nodes,
                             std::vector<int32_t>* tree_off) {
  const size_t T = tr.feat.size();
  if (tr.cond.size() != T || tr.left.size() != T || tr.right.size() != T ||
      tr.defl.size() != T || tr.leaf.size() != T)
    throw std::invalid_argument("forest lists differ in their number of trees");
  nodes->clear();
  tree_off->assign(1, 0);
  for (size_t t = 0; t < T; ++t) {
    const auto bad = [&] { return std::invalid_argument("malformed tree " + std::to_string(t)); };
    const int64_t nn = (int64_t)tr.feat[t].size();
    if (nn < 1 || (int64_t)tr.cond[t].size() != nn || (int64_t)tr.left[t].size() != nn ||
        (int64_t)tr.right[t].size() != nn || (int64_t)tr.defl[t].size() != nn ||
        (int64_t)tr.leaf[t].size() != nn || (int64_t)nodes->size() + nn > INT32_MAX)
      throw bad();
    for (int64_t i = 0; i < nn; ++i) {
      const int64_t f = tr.feat[t][i];
      if (f < 0) {
        nodes->push_back({-1, (float)tr.leaf[t][i], 0, 0});
        continue;
      }
      const int64_t l = tr.left[t][i], r = tr.right[t][i];
      if (f >= (1 << 30) || l <= i || r <= i || l >= nn || r >= nn) throw bad();
      nodes->push_back({(int32_t)(f << 1 | (tr.defl[t][i] != 0)), (float)tr.cond[t][i],
                        (int32_t)l, (int32_t)r});
    }
    tree_off->push_back((int32_t)nodes->size());
  }
}

// Consecutive whole trees [first_tree, first_tree + ntree) whose nodes
// [node_begin, node_begin + nnode) the kernel walks in one launch: from LDS
// (in_lds), or, a single tree larger than the LDS capacity, from global memory.
struct GbdtForestChunk {
  int64_t first_tree, ntree, node_begin, nnode;
  bool in_lds;
  bool operator==(const GbdtForestChunk& o) const {
    return first_tree == o.first_tree && ntree == o.ntree && node_begin == o.node_begin &&
           nnode == o.nnode && in_lds == o.in_lds;
  }
};

// Chunks in tree order that cover every tree once: each takes as many whole
// trees as fit in lds_nodes; a tree that does not fit on its own is a chunk
// of its own with in_lds = false.
inline std::vector<GbdtForestChunk> gbdt_forest_plan(const std::vector<int64_t>& tree_sizes,
                                                     int64_t lds_nodes) {
  std::vector<GbdtForestChunk> chunks;
  int64_t node = 0;
  bool open = false;  // the last chunk may still take trees
  for (int64_t t = 0; t < (int64_t)tree_sizes.size(); ++t) {
    const int64_t sz = tree_sizes[t];
    if (sz > lds_nodes) {
      chunks.push_back({t, 1, node, sz, false});
      open = false;
    } else if (open && chunks.back().nnode + sz <= lds_nodes) {
      chunks.back().ntree += 1;
      chunks.back().nnode += sz;
    } else {
      chunks.push_back({t, 1, node, sz, true});
      open = true;
    }
    node += sz;
  }
  return chunks;
}

}  // namespace wh
