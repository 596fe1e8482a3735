// Stand-alone test of the interaction references (csrc/host/
// gbdt_shap_plan.h: gbdt_shap_inter_path, gbdt_shap_inter_rows) against an
// enumeration, in this program, of the Shapley interaction index over the
// subsets of a tree's features: no torch, no HIP. build_native.py builds it
// plain (bin/native/) and under -fsanitize=address,undefined
// (--sanitize-shap-inter); exit status 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <random>

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
  // grows node i of tree t at random: an inner node with probability p
  void grow(int t, int i, int depth, int nfeat, double p, std::mt19937* rng) {
    std::uniform_real_distribution<double> u(0, 1), frac(0.1, 0.9);
    std::uniform_int_distribution<int> feat(0, nfeat - 1), grid(-4, 4);
    if (depth == 0 || u(*rng) >= p) {
      tr.leaf[t][i] = (float)(2 * u(*rng) - 1);
      return;
    }
    const double c = cover[t][i], f = frac(*rng);
    const int l = add_node(t, c * f), r = add_node(t, c * (1 - f));
    tr.feat[t][i] = feat(*rng), tr.cond[t][i] = 0.25 * grid(*rng), tr.defl[t][i] = (*rng)() & 1;
    tr.left[t][i] = l, tr.right[t][i] = r;
    grow(t, l, depth - 1, nfeat, p, rng);
    grow(t, r, depth - 1, nfeat, p, rng);
  }
  void tree(int depth, int nfeat, double p, std::mt19937* rng) {
    const int t = add_tree();
    grow(t, add_node(t, 100.0), depth, nfeat, p, rng);
  }
};

// v(S) of tree t for row r: the features whose bit is set in S are known
double game(const wh::GbdtShapModel& m, const wh::ShapDenseRows& rows, int64_t r, int t,
            unsigned S, int i = 0) {
  const int64_t o = m.tree_off[t];
  const wh::GbdtForestNode& q = m.nodes[o + i];
  if (q.fd < 0) return q.v;
  if (S >> (q.fd >> 1) & 1u) {
    float v;
    const bool left = rows.value(r, q.fd >> 1, &v) ? v < q.v : (q.fd & 1) != 0;
    return game(m, rows, r, t, S, left ? q.left : q.right);
  }
  return m.node_rl[o + i] * game(m, rows, r, t, S, q.left) +
         m.node_rr[o + i] * game(m, rows, r, t, S, q.right);
}

double fact(int k) { return k <= 1 ? 1.0 : k * fact(k - 1); }

// [K, n, F + 1, F + 1] by the definition; features are their own columns
// (every one of the F features must be used by some tree)
std::vector<double> enumerate(const wh::GbdtShapModel& m, const wh::ShapDenseRows& rows, int64_t n,
                              int F, double base) {
  const int F1 = F + 1;
  std::vector<double> out((size_t)m.K * n * F1 * F1, 0.0);
  for (int k = 0; k < m.K; ++k)
    for (int64_t r = 0; r < n; ++r) out[((k * n + r) * F1 + F) * F1 + F] = base;
  for (int t = 0; t < (int)m.ntree(); ++t) {
    unsigned N = 0;  // the tree's features
    for (int64_t i = m.tree_off[t]; i < m.tree_off[t + 1]; ++i)
      if (m.nodes[i].fd >= 0) N |= 1u << (m.nodes[i].fd >> 1);
    const int u = __builtin_popcount(N);
    for (int64_t r = 0; r < n; ++r) {
      double* o = out.data() + ((t % m.K) * n + r) * F1 * F1;
      std::vector<double> v(1u << F, 0.0), phi(F, 0.0);
      for (unsigned S = 0; S < (1u << F); ++S)
        if ((S & ~N) == 0) v[S] = game(m, rows, r, t, S);
      o[F * F1 + F] += v[0];
      for (int i = 0; i < F; ++i) {
        if (!(N >> i & 1u)) continue;
        for (unsigned S = 0; S < (1u << F); ++S) {
          if ((S & ~N) != 0 || (S >> i & 1u)) continue;
          const int s = __builtin_popcount(S);
          phi[i] += fact(s) * fact(u - s - 1) / fact(u) * (v[S | 1u << i] - v[S]);
        }
      }
      for (int i = 0; i < F; ++i) {
        double off = 0;
        for (int j = 0; j < F; ++j) {
          if (j == i || !(N >> i & 1u) || !(N >> j & 1u)) continue;
          double x = 0;
          for (unsigned S = 0; S < (1u << F); ++S) {
            if ((S & ~N) != 0 || (S >> i & 1u) || (S >> j & 1u)) continue;
            const int s = __builtin_popcount(S);
            x += fact(s) * fact(u - s - 2) / (2 * fact(u - 1)) *
                 (v[S | 1u << i | 1u << j] - v[S | 1u << i] - v[S | 1u << j] + v[S]);
          }
          o[i * F1 + j] += x;
          off += x;
        }
        o[i * F1 + i] += phi[i] - off;
      }
    }
  }
  return out;
}

void check(const Forest& f, int K, int F, int64_t n, std::mt19937* rng) {
  const auto m = wh::gbdt_shap_pack(f.tr, f.cover, K);
  EXPECT((int)m.used.size() == F);  // compact columns are the features
  if ((int)m.used.size() != F) return;
  std::vector<float> X(n * F);
  std::uniform_int_distribution<int> grid(-5, 5);
  for (auto& v : X) v = grid(*rng) == 5 ? std::nanf("") : 0.25f * grid(*rng);
  const wh::ShapDenseRows rows{X.data(), F};
  const int F1 = F + 1;
  const auto want = enumerate(m, rows, n, F, 0.25);
  std::vector<double> got(want.size(), -7.0), phi((size_t)K * n * F1);
  std::vector<float> g32(want.size(), -7.f);
  wh::gbdt_shap_inter_rows<double>(m, rows, n, 0.25, got.data());
  wh::gbdt_shap_inter_rows<float>(m, rows, n, 0.25, g32.data());
  wh::gbdt_shap_rows<double>(m, rows, n, 0.25, false, phi.data());
  for (int64_t kr = 0; kr < K * n; ++kr) {
    const double* g = got.data() + kr * F1 * F1;
    for (int i = 0; i < F1; ++i) {
      double sum = 0;
      for (int j = 0; j < F1; ++j) {
        const size_t at = (kr * F1 + i) * F1 + j;
        EXPECT(std::fabs(got[at] - want[at]) <= 1e-12);
        EXPECT(std::fabs(g32[at] - want[at]) <= 1e-5);
        EXPECT(g[i * F1 + j] == g[j * F1 + i]);  // the same number
        EXPECT(g32[at] == g32[(kr * F1 + j) * F1 + i]);
        if ((i == F) != (j == F)) EXPECT(g[i * F1 + j] == 0);
        sum += g[i * F1 + j];
      }
      EXPECT(std::fabs(sum - phi[kr * F1 + i]) <= 1e-12);  // a row sums to the contribution
    }
    EXPECT(g[F * F1 + F] == phi[kr * F1 + F]);
  }
}

}  // namespace

int main() {
  std::mt19937 rng(11);
  EXPECT(wh::gbdt_shap_inter_pairs(0) == 0 && wh::gbdt_shap_inter_pairs(1) == 0);
  EXPECT(wh::gbdt_shap_inter_pairs(2) == 1 && wh::gbdt_shap_inter_pairs(32) == 496);
  EXPECT(wh::gbdt_shap_inter_lds_cols() >= 29);  // 28 features

  // random forests over 5 features, repeated features on a path, K = 1 and 3
  for (int K : {1, 3}) {
    Forest f;
    for (int t = 0; t < 7; ++t) f.tree(4, 5, 0.85, &rng);
    f.tree(0, 5, 0.0, &rng);  // a single leaf
    f.tree(5, 5, 1.0, &rng);  // full: every feature is used
    check(f, K, 5, 9, &rng);
  }
  // one feature only: everything is on the diagonal
  {
    Forest f;
    f.tree(3, 1, 1.0, &rng);
    check(f, 1, 1, 6, &rng);
  }
  // two features: one pair
  {
    Forest f;
    f.tree(4, 2, 1.0, &rng);
    check(f, 1, 2, 6, &rng);
  }
  // a path of one element adds nothing, whatever the accumulator holds
  {
    std::vector<double> tri(3, 1.5), w;
    const wh::GbdtShapElem e{0, 2, 0.f, 1.f, 0.5, true};
    const uint8_t one = 1;
    wh::gbdt_shap_inter_path<double>(&e, 1, 2.0, &one, tri.data(), &w);
    EXPECT(tri[0] == 1.5 && tri[1] == 1.5 && tri[2] == 1.5);
  }
  // no rows, no trees
  {
    Forest f;
    const auto m = wh::gbdt_shap_pack(f.tr, f.cover, 2);
    std::vector<double> out(2 * 3, -1.0);
    const wh::ShapDenseRows rows{nullptr, 0};
    wh::gbdt_shap_inter_rows<double>(m, rows, 3, 0.5, out.data());
    for (double v : out) EXPECT(v == 0.5);  // [2, 3, 1, 1]: the bias
    wh::gbdt_shap_inter_rows<double>(m, rows, 0, 0.5, out.data());
  }

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("gbdt_shap_inter_test: ok\n");
  return 0;
}
