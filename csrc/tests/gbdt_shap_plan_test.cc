// Stand-alone test of the contribution tables and plan (csrc/host/
// gbdt_shap_plan.h): no torch, no HIP. build_native.py builds it plain
// (bin/native/) and under -fsanitize=address,undefined (--sanitize-shap-plan);
// exit status 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "host/gbdt_shap_plan.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

struct Forest {
  wh::GbdtForestTrees tr;
  std::vector<std::vector<double>> cover;
  int add_tree() {
    tr.feat.emplace_back(), tr.left.emplace_back(), tr.right.emplace_back();
    tr.defl.emplace_back(), tr.cond.emplace_back(), tr.leaf.emplace_back(), cover.emplace_back();
    return (int)tr.feat.size() - 1;
  }
  int add_node(int t, double cov) {
    tr.feat[t].push_back(-1), tr.left[t].push_back(0), tr.right[t].push_back(0);
    tr.defl[t].push_back(0), tr.cond[t].push_back(0), tr.leaf[t].push_back(0);
    cover[t].push_back(cov);
    return (int)tr.feat[t].size() - 1;
  }
  // node i of tree t becomes an inner node; returns its left child
  int split(int t, int i, int feat, double cond, int defl, double frac) {
    const double c = cover[t][i];
    const int l = add_node(t, c * frac), r = add_node(t, c * (1 - frac));
    tr.feat[t][i] = feat, tr.cond[t][i] = cond, tr.defl[t][i] = defl;
    tr.left[t][i] = l, tr.right[t][i] = r;
    return l;
  }
};

// a chain of `depth` inner nodes going left, node k on feature k % nfeat
void chain(Forest* f, int depth, int nfeat, std::mt19937* rng) {
  std::uniform_real_distribution<double> frac(0.1, 0.9), val(-1, 1);
  const int t = f->add_tree();
  int i = f->add_node(t, 100.0);
  for (int k = 0; k < depth; ++k) {
    const int l = f->split(t, i, k % nfeat, val(*rng), k & 1, frac(*rng));
    f->tr.leaf[t][l + 1] = val(*rng);
    i = l;
  }
  f->tr.leaf[t][i] = val(*rng);
}

template <class E>
bool throws_with(const char* what, E fn) {
  try {
    fn();
  } catch (const std::invalid_argument& e) {
    return std::string(e.what()).find(what) != std::string::npos;
  }
  return false;
}

void check_plan(const std::vector<int32_t>& len, const std::vector<int32_t>& cls, int64_t cap) {
  const std::vector<int32_t> tree(len.size(), 0);
  const auto plan = wh::gbdt_shap_plan(len, cls, tree, cap);
  std::set<int32_t> seen;
  int64_t path = 0, elem = 0;
  for (auto& c : plan.chunks) {
    EXPECT(c.path_begin == path && c.elem_begin == elem && c.npath >= 1);
    EXPECT(c.nelem <= cap);
    int64_t sum = 0;
    for (int64_t k = c.path_begin; k < c.path_begin + c.npath; ++k) {
      const int32_t p = plan.order[k];
      EXPECT(seen.insert(p).second);
      EXPECT(cls[p] == c.cls && wh::gbdt_shap_width(len[p]) == c.width);
      sum += len[p];
    }
    EXPECT(sum == c.nelem);
    path += c.npath, elem += c.nelem;
  }
  EXPECT(seen.size() == len.size() && path == (int64_t)len.size());
  // chunks of one class and width stay in the order the paths were given
  for (size_t k = 1; k < plan.order.size(); ++k) {
    const int32_t a = plan.order[k - 1], b = plan.order[k];
    if (cls[a] == cls[b] && wh::gbdt_shap_width(len[a]) == wh::gbdt_shap_width(len[b]))
      EXPECT(a < b);
  }
}

}  // namespace

int main() {
  std::mt19937 rng(5);
  // widths
  EXPECT(wh::gbdt_shap_width(1) == 16 && wh::gbdt_shap_width(15) == 16);
  EXPECT(wh::gbdt_shap_width(16) == 32 && wh::gbdt_shap_width(31) == 32);
  EXPECT(wh::gbdt_shap_width(32) == 64 && wh::gbdt_shap_width(63) == 64);
  EXPECT(wh::gbdt_shap_width(64) == 0);

  // merging: a chain of depth 12 over 3 features has paths of at most 3
  // elements whose z is the product of its nodes' ratios
  {
    Forest f;
    chain(&f, 12, 3, &rng);
    f.add_tree();
    f.add_node(1, 3.0);  // a single leaf: no path
    f.tr.leaf[1][0] = 0.5;
    const auto m = wh::gbdt_shap_pack(f.tr, f.cover, 1);
    EXPECT(m.used.size() == 3 && m.paths.size() == 13 && m.tree_E.size() == 2);
    EXPECT(m.tree_E[1] == 0.5);
    double E = 0;
    for (auto& p : m.paths) {
      EXPECT(p.len >= 1 && p.len <= 3 && p.tree == 0);
      double z = 1;
      std::set<int32_t> cols;
      for (int k = p.begin; k < p.begin + p.len; ++k) {
        const auto& e = m.elems[k];
        EXPECT(cols.insert(e.col).second && m.used[e.col] == e.feat);
        EXPECT(e.z > 0 && e.z < 1);
        z *= e.z;
      }
      E += z * p.leaf;
    }
    EXPECT(std::fabs(E - m.tree_E[0]) < 1e-12);
    // every row's contributions and bias sum to the leaf it reaches
    std::vector<float> X(5 * 3);
    std::uniform_real_distribution<float> val(-1, 1);
    for (auto& v : X) v = val(rng);
    X[4] = X[7] = std::nanf("");
    std::vector<double> out(5 * 4), sa(5 * 4);
    const wh::ShapDenseRows rows{X.data(), 3};
    wh::gbdt_shap_rows<double>(m, rows, 5, 0.25, false, out.data());
    wh::gbdt_shap_rows<double>(m, rows, 5, 0.25, true, sa.data());
    std::vector<float> o32(5 * 4);
    wh::gbdt_shap_rows<float>(m, rows, 5, 0.25, false, o32.data());
    for (int r = 0; r < 5; ++r) {
      int i = 0;
      while (m.nodes[i].fd >= 0) {
        float v;
        const bool left = rows.value(r, m.nodes[i].fd >> 1, &v) ? v < m.nodes[i].v
                                                                 : (m.nodes[i].fd & 1) != 0;
        i = left ? m.nodes[i].left : m.nodes[i].right;
      }
      const double want = 0.25 + m.nodes[i].v + 0.5;
      double s = 0, s2 = 0;
      for (int c = 0; c < 4; ++c) s += out[r * 4 + c], s2 += sa[r * 4 + c];
      EXPECT(std::fabs(s - want) < 1e-12 && std::fabs(s2 - want) < 1e-12);
      EXPECT(std::fabs(out[r * 4 + 3] - (0.25 + m.tree_E[0] + 0.5)) < 1e-12);
      for (int c = 0; c < 4; ++c) EXPECT(std::fabs(o32[r * 4 + c] - out[r * 4 + c]) < 1e-5);
    }
    // the table follows the plan's order
    const auto plan = wh::gbdt_shap_plan(m, 64);
    const auto tab = wh::gbdt_shap_table(m, plan);
    EXPECT(tab.paths.size() == 4 * m.paths.size() && tab.elems.size() == 4 * m.elems.size());
    EXPECT(tab.ecol.size() == m.elems.size() && plan.chunks.size() >= 1);
    int32_t at = 0;
    for (size_t k = 0; k < plan.order.size(); ++k) {
      EXPECT(tab.paths[4 * k] == at && tab.paths[4 * k + 1] == m.paths[plan.order[k]].len);
      at += tab.paths[4 * k + 1];
    }
  }

  // plan invariants around the capacity, classes and widths mixed
  {
    std::uniform_int_distribution<int> len(1, 63), cls(0, 2);
    for (int64_t cap : {63, 64, 100, 2048})
      for (int n : {0, 1, 2, 50, 400}) {
        std::vector<int32_t> l(n), c(n);
        for (int k = 0; k < n; ++k) l[k] = len(rng), c[k] = cls(rng);
        check_plan(l, c, cap);
      }
    check_plan({15, 15, 15, 15}, {0, 0, 0, 0}, 63);       // exactly full, then a new chunk
    check_plan({31, 32, 31, 32, 1}, {0, 0, 0, 0, 0}, 63);  // widths alternate
    check_plan(std::vector<int32_t>(130, 1), std::vector<int32_t>(130, 0), 64);
  }

  // refusals
  {
    Forest f;
    chain(&f, 3, 3, &rng);
    chain(&f, 64, 64, &rng);
    const auto m = wh::gbdt_shap_pack(f.tr, f.cover, 1);  // the host takes any length
    int longest = 0;
    for (auto& p : m.paths) longest = std::max(longest, (int)p.len);
    EXPECT(longest == 64);
    EXPECT(throws_with("tree 1 has a path of 64", [&] { wh::gbdt_shap_plan(m); }));
    EXPECT(throws_with("capacity", [&] { wh::gbdt_shap_plan({1}, {0}, {0}, 62); }));
    EXPECT(throws_with("empty path", [&] { wh::gbdt_shap_plan({0}, {0}, {0}, 64); }));
    Forest g;
    chain(&g, 2, 2, &rng);
    chain(&g, 2, 2, &rng);
    for (double bad : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
      auto cover = g.cover;
      cover[1][3] = bad;
      EXPECT(throws_with("tree 1 has no usable cover statistics",
                         [&] { wh::gbdt_shap_pack(g.tr, cover, 1); }));
    }
    auto cover = g.cover;
    cover[0].pop_back();
    EXPECT(throws_with("malformed tree 0", [&] { wh::gbdt_shap_pack(g.tr, cover, 1); }));
    EXPECT(throws_with("classes", [&] { wh::gbdt_shap_pack(g.tr, g.cover, 0); }));
  }

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("gbdt_shap_plan_test: ok\n");
  return 0;
}
