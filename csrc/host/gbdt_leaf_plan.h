// Best-first (grow_policy=lossguide) tree growth, its bookkeeping: the limits
// that max_leaves and max_depth put into effect, the rule that picks the next
// leaf to split, the ids and histogram slots of a split's children, and the
// tree lists of the device loop's node table. Free of HIP and torch: the
// binding compiles it and a CPU-only machine can call it.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

#include "host/gbdt_dart_plan.h"
#include "host/gbdt_shap_plan.h"

namespace wh {

// A tree of L leaves has 2 L - 1 nodes; the node tables of the heap walk and
// of the dart walk hold at most 65535 of them.
constexpr int64_t kLeafMaxLeaves = 32768;
static_assert(2 * kLeafMaxLeaves - 1 <= 65535, "a lossguide tree fits a 16-bit node table");

// The deepest leaf the model's consumers admit. A leaf at depth d has a SHAP
// path of d + 1 elements (the root's dummy element included), at most
// kShapMaxPath; the dart walk takes at most kDartMaxDepth steps, so a leaf at
// depth kDartMaxDepth at the deepest. The smaller of the two: 62.
constexpr int kLeafDepthCap = std::min(kShapMaxPath - 1, kDartMaxDepth);
inline int64_t gbdt_leaf_depth_cap() { return kLeafDepthCap; }

// What max_leaves and max_depth put into effect under lossguide: the tree
// stops at `leaves` leaves and a node at depth `depth` is never split. error:
// nullptr, or why the pair is refused (it names the parameter).
struct GbdtLeafLimits {
  int64_t leaves, depth;
  const char* error;
};

// max_leaves in [0, kLeafMaxLeaves] (0: no limit of its own), max_depth >= 0
// (0: no depth limit, the cap above holds; a larger value than the cap is the
// cap). Without max_leaves a depth limit D gives min(2^D, kLeafMaxLeaves)
// leaves; neither limit is an error.
inline GbdtLeafLimits gbdt_leaf_limits(int64_t max_leaves, int64_t max_depth) {
  if (max_leaves < 0 || max_leaves > kLeafMaxLeaves)
    return {0, 0, "max_leaves must be an integer in [0, 32768]"};
  if (max_depth < 0) return {0, 0, "max_depth must not be negative"};
  if (max_leaves == 0 && max_depth == 0)
    return {0, 0, "grow_policy=lossguide needs max_leaves > 0 or max_depth > 0"};
  const int64_t depth = max_depth > 0 ? std::min<int64_t>(max_depth, kLeafDepthCap) : kLeafDepthCap;
  int64_t leaves = max_leaves;
  if (leaves == 0) leaves = depth >= 15 ? kLeafMaxLeaves : std::min(int64_t{1} << depth, kLeafMaxLeaves);
  return {leaves, depth, nullptr};
}

// An open leaf: its node id, its depth and the gain of its best split.
struct GbdtOpenLeaf {
  int64_t node, depth;
  double gain;
};

// The next leaf to split: among the open leaves with gain > rt_eps and depth <
// depth_cap the one of the largest gain, ties to the smaller node id; its
// index in `open`, or -1 when none is eligible. (A NaN gain is not eligible.)
inline int64_t gbdt_leaf_pick(const std::vector<GbdtOpenLeaf>& open, double rt_eps,
                              int64_t depth_cap) {
  int64_t best = -1;
  for (int64_t i = 0; i < (int64_t)open.size(); ++i) {
    const auto& o = open[i];
    if (!(o.gain > rt_eps) || o.depth >= depth_cap) continue;
    if (best < 0 || o.gain > open[best].gain ||
        (o.gain == open[best].gain && o.node < open[best].node))
      best = i;
  }
  return best;
}

// The children of the k-th split of a tree (k = 0, 1, ...): nodes are numbered
// in creation order, the root is 0.
inline int64_t gbdt_leaf_left(int64_t k) { return 2 * k + 1; }
inline int64_t gbdt_leaf_right(int64_t k) { return 2 * k + 2; }

// A node's histogram slot in the device loop's pool: its id, so the children
// of step k are built into slots 2k + 1 and 2k + 2 whichever leaf was picked.
// The pool of a tree of `leaves` leaves holds this many histograms.
inline int64_t gbdt_leaf_pool_slots(int64_t leaves) { return 2 * leaves - 1; }

// A grown tree as lists, nodes renumbered breadth-first from the root, and
// its leaves' row segments {leaf id, begin, end}.
struct GbdtLeafTree {
  std::vector<int> feat, bin, defl, left, right, parent;
  std::vector<double> gain, cover, bw, leaf;
  std::vector<std::array<int, 3>> segs;
};

// The tree of a table of explicit-child node records r [nn x rec] (rec >= 10
// doubles: {left child id or -1 (right = left + 1), feat, bin, defl, gain,
// cover, base weight, leaf, begin, end}), walked from node 0; a step that
// split nothing left two records nobody points to, and they are dropped.
// False when the table is no tree: a child id that does not grow along the
// walk or lies past the table (so no node is reached twice), or a split
// without a feature.
inline bool gbdt_leaf_tree_lists(const double* r, int64_t nn, int rec, GbdtLeafTree* t) {
  *t = GbdtLeafTree();
  if (nn < 1 || rec < 10) return false;
  std::vector<int64_t> order{0}, parent{-1};
  for (size_t i = 0; i < order.size(); ++i) {
    const int64_t h = order[i];
    const double* q = r + h * rec;
    const int64_t l = (int64_t)q[0];
    if (l < 0) continue;
    // children are made after their parent, two per step: ids grow, so the
    // walk ends and reaches a node once (a node has one pair of children ids,
    // and a pair belongs to one step)
    if (l <= h || l + 1 >= nn || l % 2 != 1 || !(q[1] >= 0.0)) return false;
    if ((int64_t)order.size() + 2 > nn) return false;
    order.push_back(l), order.push_back(l + 1);
    parent.push_back((int64_t)i), parent.push_back((int64_t)i);
  }
  const size_t m = order.size();
  std::vector<int> id_of(nn, -1);
  for (size_t i = 0; i < m; ++i) {
    if (id_of[order[i]] >= 0) return false;  // reached twice
    id_of[order[i]] = (int)i;
  }
  t->feat.assign(m, -1), t->bin.assign(m, 0), t->defl.assign(m, 0), t->left.assign(m, -1);
  t->right.assign(m, -1), t->parent.assign(m, -1), t->gain.assign(m, 0.0);
  t->cover.assign(m, 0.0), t->bw.assign(m, 0.0), t->leaf.assign(m, 0.0);
  for (size_t i = 0; i < m; ++i) {
    const double* q = r + order[i] * rec;
    t->parent[i] = (int)parent[i];
    t->cover[i] = q[5], t->bw[i] = q[6], t->leaf[i] = q[7];
    if ((int64_t)q[0] >= 0) {
      t->feat[i] = (int)q[1], t->bin[i] = (int)q[2], t->defl[i] = (int)q[3], t->gain[i] = q[4];
      t->left[i] = id_of[(int64_t)q[0]], t->right[i] = id_of[(int64_t)q[0] + 1];
    } else {
      t->segs.push_back({(int)i, (int)q[8], (int)q[9]});
    }
  }
  return true;
}

}  // namespace wh
