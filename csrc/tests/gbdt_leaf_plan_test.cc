// Stand-alone test of the best-first growth bookkeeping
// (csrc/host/gbdt_leaf_plan.h): no torch, no HIP. build_native.py builds it
// plain (bin/native/) and under -fsanitize=address,undefined
// (--sanitize-leaf-plan); exit status 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "host/gbdt_leaf_plan.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

bool refused(int64_t leaves, int64_t depth, const char* names) {
  const auto l = wh::gbdt_leaf_limits(leaves, depth);
  return l.error != nullptr && std::strstr(l.error, names) != nullptr;
}

void test_limits() {
  // the cap follows the consumers' constants: a leaf's SHAP path and the dart walk
  EXPECT(wh::gbdt_leaf_depth_cap() == 62);
  EXPECT(wh::gbdt_leaf_depth_cap() + 1 <= wh::kShapMaxPath);
  EXPECT(wh::gbdt_leaf_depth_cap() <= wh::kDartMaxDepth);
  auto l = wh::gbdt_leaf_limits(255, 0);
  EXPECT(!l.error && l.leaves == 255 && l.depth == 62);
  l = wh::gbdt_leaf_limits(20, 5);
  EXPECT(!l.error && l.leaves == 20 && l.depth == 5);
  l = wh::gbdt_leaf_limits(0, 5);
  EXPECT(!l.error && l.leaves == 32 && l.depth == 5);
  l = wh::gbdt_leaf_limits(0, 15);
  EXPECT(!l.error && l.leaves == 32768 && l.depth == 15);
  l = wh::gbdt_leaf_limits(0, 40);  // 2^40 leaves: the table's limit
  EXPECT(!l.error && l.leaves == 32768 && l.depth == 40);
  l = wh::gbdt_leaf_limits(0, 1000);  // (no shift by 1000)
  EXPECT(!l.error && l.leaves == 32768 && l.depth == 62);
  l = wh::gbdt_leaf_limits(32768, 63);
  EXPECT(!l.error && l.leaves == 32768 && l.depth == 62);
  l = wh::gbdt_leaf_limits(1, 0);  // a single leaf: the root is never split
  EXPECT(!l.error && l.leaves == 1);
  EXPECT(refused(32769, 0, "max_leaves"));
  EXPECT(refused(-1, 3, "max_leaves"));
  EXPECT(refused(8, -1, "max_depth"));
  EXPECT(refused(0, 0, "max_leaves") && refused(0, 0, "max_depth"));
}

void test_pick() {
  using L = wh::GbdtOpenLeaf;
  const double eps = 1e-6;
  EXPECT(wh::gbdt_leaf_pick({}, eps, 62) == -1);
  EXPECT(wh::gbdt_leaf_pick({L{0, 0, 3.0}}, eps, 62) == 0);
  EXPECT(wh::gbdt_leaf_pick({L{0, 0, eps}}, eps, 62) == -1);  // gain > eps, strictly
  EXPECT(wh::gbdt_leaf_pick({L{0, 0, -INFINITY}}, eps, 62) == -1);
  EXPECT(wh::gbdt_leaf_pick({L{0, 0, std::numeric_limits<double>::quiet_NaN()}}, eps, 62) == -1);
  // the largest gain, wherever it stands
  EXPECT(wh::gbdt_leaf_pick({L{3, 2, 1.0}, L{4, 2, 5.0}, L{2, 1, 2.0}}, eps, 62) == 1);
  // ties: the smaller node id, in either order of the table
  EXPECT(wh::gbdt_leaf_pick({L{7, 3, 2.5}, L{4, 2, 2.5}, L{9, 4, 2.5}}, eps, 62) == 1);
  EXPECT(wh::gbdt_leaf_pick({L{4, 2, 2.5}, L{7, 3, 2.5}}, eps, 62) == 0);
  // a leaf at the depth cap is passed over, whatever its gain
  EXPECT(wh::gbdt_leaf_pick({L{3, 5, 9.0}, L{4, 4, 1.0}}, eps, 5) == 1);
  EXPECT(wh::gbdt_leaf_pick({L{3, 5, 9.0}, L{4, 5, 1.0}}, eps, 5) == -1);
  // against a plain reference on random tables with many ties
  std::mt19937 rng(5);
  for (int it = 0; it < 2000; ++it) {
    std::vector<L> open;
    const int m = rng() % 12;
    for (int i = 0; i < m; ++i)
      open.push_back(L{(int64_t)(rng() % 40), (int64_t)(rng() % 6), (double)(rng() % 4) - 1.0});
    int64_t want = -1;
    for (int64_t i = 0; i < m; ++i) {
      if (open[i].gain <= eps || open[i].depth >= 4) continue;
      if (want < 0 || open[i].gain > open[want].gain) want = i;
    }
    const int64_t got = wh::gbdt_leaf_pick(open, eps, 4);
    EXPECT((got < 0) == (want < 0));
    if (got >= 0 && want >= 0) {
      EXPECT(open[got].gain == open[want].gain && open[got].depth < 4);
      for (const auto& o : open)  // no eligible leaf of that gain has a smaller id
        EXPECT(!(o.gain == open[got].gain && o.depth < 4 && o.node < open[got].node));
    }
  }
}

void test_ids() {
  // creation order: step k makes nodes 2k + 1 and 2k + 2, so L leaves end at 2L - 2
  for (int64_t k = 0; k < 5; ++k) {
    EXPECT(wh::gbdt_leaf_left(k) == 2 * k + 1 && wh::gbdt_leaf_right(k) == 2 * k + 2);
  }
  EXPECT(wh::gbdt_leaf_right(wh::kLeafMaxLeaves - 2) == 65534);  // the last id of a full table
}

// records of a tree grown in three steps, the second of them idle:
//   0 splits (step 0) into 1, 2; step 1 idle (3, 4 unreachable); 2 splits
//   (step 2) into 5, 6
std::vector<double> records() {
  const int rec = 10;
  std::vector<double> r(7 * rec, 0.0);
  auto set = [&](int i, double left, double feat, double bin, double defl, double gain,
                 double cover, double bw, double leaf, double b, double e) {
    const double v[10] = {left, feat, bin, defl, gain, cover, bw, leaf, b, e};
    for (int j = 0; j < rec; ++j) r[i * rec + j] = v[j];
  };
  set(0, 1, 3, 7, 1, 9.5, 100, 0.1, 0.05, 0, 100);
  set(1, -1, -1, 0, 0, 0, 40, 0.2, 0.10, 0, 40);
  set(2, 5, 0, 2, 0, 4.5, 60, 0.3, 0.15, 40, 100);
  set(3, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0);
  set(4, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0);
  set(5, -1, -1, 0, 0, 0, 25, 0.4, 0.20, 40, 65);
  set(6, -1, -1, 0, 0, 0, 35, 0.5, 0.25, 65, 100);
  return r;
}

void test_tree_lists() {
  EXPECT(wh::gbdt_leaf_pool_slots(1) == 1 && wh::gbdt_leaf_pool_slots(256) == 511);
  wh::GbdtLeafTree t;
  auto r = records();
  EXPECT(wh::gbdt_leaf_tree_lists(r.data(), 7, 10, &t));
  EXPECT((t.feat == std::vector<int>{3, -1, 0, -1, -1}));
  EXPECT((t.bin == std::vector<int>{7, 0, 2, 0, 0}));
  EXPECT((t.defl == std::vector<int>{1, 0, 0, 0, 0}));
  EXPECT((t.left == std::vector<int>{1, -1, 3, -1, -1}));
  EXPECT((t.right == std::vector<int>{2, -1, 4, -1, -1}));
  EXPECT((t.parent == std::vector<int>{-1, 0, 0, 2, 2}));
  EXPECT((t.gain == std::vector<double>{9.5, 0, 4.5, 0, 0}));
  EXPECT((t.cover == std::vector<double>{100, 40, 60, 25, 35}));
  EXPECT((t.leaf == std::vector<double>{0.05, 0.10, 0.15, 0.20, 0.25}));
  EXPECT(t.segs.size() == 3 && (t.segs[0] == std::array<int, 3>{1, 0, 40}) &&
         (t.segs[1] == std::array<int, 3>{3, 40, 65}) &&
         (t.segs[2] == std::array<int, 3>{4, 65, 100}));
  // a single leaf
  EXPECT(wh::gbdt_leaf_tree_lists(r.data() + 10, 1, 10, &t) && t.feat.size() == 1 &&
         t.segs.size() == 1);
  // what is no tree
  EXPECT(!wh::gbdt_leaf_tree_lists(r.data(), 0, 10, &t));
  EXPECT(!wh::gbdt_leaf_tree_lists(r.data(), 7, 9, &t));
  EXPECT(!wh::gbdt_leaf_tree_lists(r.data(), 6, 10, &t));  // node 2's right child past the table
  auto bad = r;
  bad[2 * 10] = 1;  // node 2 points back at node 0's children
  EXPECT(!wh::gbdt_leaf_tree_lists(bad.data(), 7, 10, &t));
  bad = r;
  bad[2 * 10] = 4;  // an even left child id
  EXPECT(!wh::gbdt_leaf_tree_lists(bad.data(), 7, 10, &t));
  bad = r;
  bad[1 * 10] = 5;  // two parents of one pair (and no feature)
  EXPECT(!wh::gbdt_leaf_tree_lists(bad.data(), 7, 10, &t));
  bad[1 * 10 + 1] = 2;  // ... with a feature: node 5 is reached twice
  EXPECT(!wh::gbdt_leaf_tree_lists(bad.data(), 7, 10, &t));
}

}  // namespace

int main() {
  test_tree_lists();
  test_limits();
  test_pick();
  test_ids();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::puts("gbdt_leaf_plan_test: ok");
  return 0;
}
