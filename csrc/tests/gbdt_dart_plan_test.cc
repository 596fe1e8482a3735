// Stand-alone test of the DART tree table and walk plan
// (csrc/host/gbdt_dart_plan.h): no torch, no HIP. build_native.py builds it
// plain (bin/native/) and under -fsanitize=address,undefined
// (--sanitize-dart-plan); exit status 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "host/gbdt_dart_plan.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// a full binary tree of the given depth in BFS order, node i splitting on
// feature i % F at bin i % 7
wh::GbdtDartTree full_tree(int depth, int F) {
  wh::GbdtDartTree t;
  const int nn = (1 << (depth + 1)) - 1, inner = (1 << depth) - 1;
  for (int i = 0; i < nn; ++i) {
    const bool leaf = i >= inner;
    t.feat.push_back(leaf ? -1 : i % F);
    t.bin.push_back(leaf ? 0 : i % 7);
    t.cond.push_back(0.0);
    t.left.push_back(leaf ? -1 : 2 * i + 1);
    t.right.push_back(leaf ? -1 : 2 * i + 2);
    t.defl.push_back(i & 1);
    t.leaf.push_back(leaf ? 0.25 * i : 0.0);
  }
  return t;
}

// F features of 8 cuts each: 0.5, 1.5, ...
void cuts(int F, std::vector<double>* vals, std::vector<int64_t>* off) {
  off->assign(1, 0);
  for (int f = 0; f < F; ++f) {
    for (int b = 0; b < 8; ++b) vals->push_back(b + 0.5 + 0.001 * f);
    off->push_back((int64_t)vals->size());
  }
}

// every selected tree once, in order; staged chunks within both budgets with
// contiguous staging offsets; unstaged ones exactly the trees that cannot be
void check_plan(const std::vector<int64_t>& sizes, const std::vector<int64_t>& sel,
                int64_t lds, int64_t max_trees) {
  const auto chunks = wh::gbdt_dart_plan(sizes, sel, lds, max_trees);
  int64_t pos = 0;
  for (size_t c = 0; c < chunks.size(); ++c) {
    const auto& ch = chunks[c];
    EXPECT(ch.first == pos && ch.count >= 1);
    if (!ch.staged) {
      const int64_t sz = sizes[sel[ch.first]];
      EXPECT(ch.count == 1 && (sz <= 0 || sz > lds) && ch.stage_off.empty());
    } else {
      EXPECT((int64_t)ch.stage_off.size() == ch.count && ch.count <= max_trees);
      int64_t off = 0;
      for (int64_t j = 0; j < ch.count; ++j) {
        const int64_t sz = sizes[sel[ch.first + j]];
        EXPECT(sz >= 1 && ch.stage_off[j] == off);
        off += sz;
      }
      EXPECT(off == ch.nnode && off <= lds);
      // greedy: the next tree, if it can be staged at all, did not fit here
      if (c + 1 < chunks.size() && chunks[c + 1].staged)
        EXPECT(ch.count == max_trees || ch.nnode + sizes[sel[chunks[c + 1].first]] > lds);
    }
    pos += ch.count;
  }
  EXPECT(pos == (int64_t)sel.size());
}

void test_plan() {
  EXPECT(wh::gbdt_dart_plan({3, 5}, {}, 16).empty());
  {  // a single stump
    const auto c = wh::gbdt_dart_plan({1}, {0}, 16);
    EXPECT(c.size() == 1 && c[0].staged && c[0].first == 0 && c[0].count == 1 && c[0].nnode == 1 &&
           c[0].stage_off == std::vector<int64_t>{0});
  }
  {  // three chunks, the last one partial; a non-contiguous selection
    const std::vector<int64_t> sizes(10, 7), sel = {0, 2, 3, 5, 6, 8, 9};
    const auto c = wh::gbdt_dart_plan(sizes, sel, 21);
    EXPECT(c.size() == 3 && c[0].count == 3 && c[1].count == 3 && c[2].count == 1 &&
           c[2].nnode == 7);
    check_plan(sizes, sel, 21, wh::kDartMaxTrees);
  }
  {  // an over-budget tree in the middle, and one that is not in the table
    const std::vector<int64_t> sizes = {7, 7, 40, 7, 0, 7}, sel = {0, 1, 2, 3, 4, 5};
    const auto c = wh::gbdt_dart_plan(sizes, sel, 21);
    EXPECT(c.size() == 5 && c[0].staged && c[0].count == 2 && !c[1].staged && c[1].first == 2 &&
           c[2].staged && c[2].count == 1 && !c[3].staged && c[3].first == 4 && c[4].staged);
    check_plan(sizes, sel, 21, wh::kDartMaxTrees);
  }
  {  // the tree cap closes a chunk of stumps
    const std::vector<int64_t> sizes(9, 1), sel = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    const auto c = wh::gbdt_dart_plan(sizes, sel, 100, 4);
    EXPECT(c.size() == 3 && c[0].count == 4 && c[2].count == 1);
  }
  bool threw = false;
  try {
    wh::gbdt_dart_plan({3}, {1}, 16);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  std::mt19937 rng(5);
  for (int it = 0; it < 200; ++it) {
    std::vector<int64_t> sizes(1 + rng() % 40), sel;
    for (auto& s : sizes) s = (int64_t)(rng() % 70) - 3;
    for (size_t t = 0; t < sizes.size(); ++t)
      if (rng() % 3) sel.push_back((int64_t)t);
    check_plan(sizes, sel, 1 + rng() % 64, 1 + rng() % 6);
  }
}

void test_pack() {
  std::vector<double> cv;
  std::vector<int64_t> co;
  cuts(5, &cv, &co);
  std::vector<wh::GbdtDartNode> nodes;
  {  // the node words
    const auto t = full_tree(2, 5);
    EXPECT(wh::gbdt_dart_pack(t, cv, co, &nodes) && nodes.size() == 7);
    EXPECT(nodes[1].w0 == (1u | 1u << 16 | 1u << 24) && nodes[1].w1 == (3u | 4u << 16));
    EXPECT(nodes[0].w0 == 0u && nodes[0].w1 == (1u | 2u << 16));
    float v;
    std::memcpy(&v, &nodes[5].w1, 4);
    EXPECT(nodes[5].w0 == wh::kDartLeaf && v == 1.25f);
  }
  {  // a stump
    wh::GbdtDartTree t{{-1}, {0}, {-1}, {-1}, {0}, {0.0}, {0.5}};
    EXPECT(wh::gbdt_dart_pack(t, cv, co, &nodes) && nodes.size() == 1);
  }
  {  // bins recovered from the cuts: an exact hit, and a cond that is no cut
    auto t = full_tree(1, 5);
    t.bin.clear();
    t.cond[0] = (double)(float)3.5;
    EXPECT(wh::gbdt_dart_pack(t, cv, co, &nodes) && ((nodes[0].w0 >> 16) & 255u) == 3u);
    t.cond[0] = 3.25;
    EXPECT(!wh::gbdt_dart_pack(t, cv, co, &nodes) && nodes.empty());
    EXPECT(wh::gbdt_dart_recover_bin(cv, co[1], co[2], (double)(float)0.501) == 0);
    EXPECT(wh::gbdt_dart_recover_bin(cv, co[1], co[2], 0.5) == -1);
    EXPECT(wh::gbdt_dart_recover_bin(cv, co[1], co[1], 0.5) == -1);
  }
  {  // the limits: bin 255, a feature past the cuts, feature 65535, 65536 nodes
    auto t = full_tree(1, 5);
    t.bin[0] = 254;
    EXPECT(wh::gbdt_dart_pack(t, cv, co, &nodes));
    t.bin[0] = 255;
    EXPECT(!wh::gbdt_dart_pack(t, cv, co, &nodes));
    t.bin[0] = 1;
    t.feat[0] = 5;
    EXPECT(!wh::gbdt_dart_pack(t, cv, co, &nodes));
    std::vector<int64_t> wide(65537, 0);  // 65536 features without cuts
    std::vector<double> none;
    t.feat[0] = 65534;
    EXPECT(wh::gbdt_dart_pack(t, none, wide, &nodes) && (nodes[0].w0 & 0xffffu) == 65534u);
    t.feat[0] = 65535;
    EXPECT(!wh::gbdt_dart_pack(t, none, wide, &nodes));
    // a right-leaning chain: 2 k + 1 nodes
    auto chain = [](int k) {
      wh::GbdtDartTree c;
      for (int i = 0; i < k; ++i) {
        c.feat.insert(c.feat.end(), {0, -1}), c.bin.insert(c.bin.end(), {1, 0});
        c.cond.insert(c.cond.end(), {0.0, 0.0}), c.defl.insert(c.defl.end(), {0, 0});
        c.left.insert(c.left.end(), {2 * i + 1, -1});
        c.right.insert(c.right.end(), {2 * i + 2, -1});
        c.leaf.insert(c.leaf.end(), {0.0, 1.0});
      }
      c.feat.push_back(-1), c.bin.push_back(0), c.cond.push_back(0.0), c.defl.push_back(0);
      c.left.push_back(-1), c.right.push_back(-1), c.leaf.push_back(2.0);
      return c;
    };
    EXPECT(wh::gbdt_dart_pack(chain(wh::kDartMaxDepth), cv, co, &nodes));
    EXPECT(!wh::gbdt_dart_pack(chain(wh::kDartMaxDepth + 1), cv, co, &nodes));  // too deep
    // 65535 nodes fit, 65536 do not (a wide shallow tree: depth 15 and 16 rows)
    auto t15 = full_tree(15, 5);  // 65535 nodes
    EXPECT(t15.feat.size() == 65535 && wh::gbdt_dart_pack(t15, cv, co, &nodes));
    t15.feat.push_back(-1), t15.bin.push_back(0), t15.cond.push_back(0.0), t15.defl.push_back(0);
    t15.left.push_back(-1), t15.right.push_back(-1), t15.leaf.push_back(0.0);
    EXPECT(t15.feat.size() == 65536 && !wh::gbdt_dart_pack(t15, cv, co, &nodes));
  }
  {  // malformed: a child before its parent, lists of different lengths
    auto t = full_tree(1, 5);
    t.left[0] = 0;
    EXPECT(!wh::gbdt_dart_pack(t, cv, co, &nodes));
    t = full_tree(1, 5);
    t.leaf.pop_back();
    EXPECT(!wh::gbdt_dart_pack(t, cv, co, &nodes));
  }
}

}  // namespace

int main() {
  test_plan();
  test_pack();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::puts("gbdt_dart_plan_test: ok");
  return 0;
}
