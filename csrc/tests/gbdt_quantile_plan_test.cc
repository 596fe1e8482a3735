// Stand-alone test of the quantile select's host parts
// (csrc/host/gbdt_quantile_plan.h): no torch, no HIP. build_native.py builds it
// plain (bin/native/) and under -fsanitize=address,undefined
// (--sanitize-quantile-plan); exit status 0 = pass.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "host/gbdt_quantile_plan.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// the definition, by brute force: min v with sum of u over r <= v >= T
bool brute(const std::vector<float>& r, const std::vector<int64_t>& u, double alpha, float* q) {
  int64_t W = 0;
  for (auto x : u) W += x;
  if (W == 0) return false;
  const int64_t T = wh::qsel_threshold(alpha, W);
  bool have = false;
  for (float v : r) {
    int64_t s = 0;
    for (size_t i = 0; i < r.size(); ++i)
      if (r[i] <= v) s += u[i];
    if (s >= T && (!have || v < *q)) *q = v, have = true;
  }
  return have;
}

// the four passes on the host: histogram of the matching keys, then the pick
bool select(const std::vector<float>& r, const std::vector<int64_t>& u, double alpha, float* q) {
  int64_t state[wh::kQselState] = {0, 0};
  for (int p = 0; p < wh::kQselPasses; ++p) {
    int64_t bins[wh::kQselBins] = {0};
    for (size_t i = 0; i < r.size(); ++i) {
      const uint32_t k = wh::qsel_key(r[i]);
      if (wh::qsel_match(k, (uint32_t)state[0], p)) bins[wh::qsel_digit(k, p)] += u[i];
    }
    EXPECT(wh::qsel_pick(bins, p, alpha, state));
  }
  *q = wh::qsel_unkey((uint32_t)state[0]);
  return state[1] != 0;
}

void test_key() {
  const float inf = std::numeric_limits<float>::infinity();
  const float v[] = {-inf, -3.4e38f, -2.f, -1.f, -1e-38f, -1e-42f, -1.4e-45f, 0.f,
                     1.4e-45f, 1e-42f, 1e-38f, 1.f, 1.0000001f, 2.f, 3.4e38f, inf};
  const int n = sizeof(v) / sizeof(v[0]);
  for (int i = 0; i < n; ++i) {
    EXPECT(wh::qsel_unkey(wh::qsel_key(v[i])) == v[i]);
    if (i) EXPECT(wh::qsel_key(v[i - 1]) < wh::qsel_key(v[i]));
  }
  EXPECT(wh::qsel_key(-0.f) == wh::qsel_key(0.f));
  EXPECT(wh::qsel_bits(wh::qsel_unkey(wh::qsel_key(-0.f))) == 0u);  // +0.0
  EXPECT(wh::qsel_digit(0x12345678u, 0) == 0x12 && wh::qsel_digit(0x12345678u, 3) == 0x78);
  EXPECT(wh::qsel_match(0x12345678u, 0xffffffffu, 0));
  EXPECT(wh::qsel_match(0x12345678u, 0x12340000u, 2) && !wh::qsel_match(0x12355678u, 0x12340000u, 2));
}

void test_weight_threshold() {
  EXPECT(wh::qsel_weight(3.f, true, 1.0) == 3 && wh::qsel_weight(3.f, false, 1.0) == 0);
  EXPECT(wh::qsel_weight(-1.f, true, 1.0) == 0 && wh::qsel_weight(0.f, true, 8.0) == 0);
  EXPECT(wh::qsel_weight(0.3f, true, 1024.0) == 307);
  EXPECT(wh::qsel_weight(0.5f, true, 1.0) == 0 && wh::qsel_weight(1.5f, true, 1.0) == 2);  // ties to even
  EXPECT(wh::qsel_scale(1.0) == 0x1p61 && wh::qsel_scale(3.0) == 0x1p59);
  EXPECT(wh::qsel_scale(0x1p61) == 1.0 && wh::qsel_scale(0.0) == 0x1p100);
  EXPECT(wh::qsel_scale(0x1p200) == 0x1p-60);
  EXPECT(wh::qsel_threshold(0.5, 4) == 2 && wh::qsel_threshold(0.5, 5) == 3);
  EXPECT(wh::qsel_threshold(0.125, 1) == 1 && wh::qsel_threshold(0.75, 8) == 6);
  EXPECT(wh::qsel_threshold(1e-30, 7) == 1);
  const int64_t big = (int64_t)1 << 61;
  EXPECT(wh::qsel_threshold(0.9999999999999999, big + 1) <= big + 1);
}

void test_select() {
  std::mt19937 g(5);
  const double alphas[] = {0.5, 0.25, 0.75, 0.125, 0.1, 0.9};
  for (int n : {1, 2, 3, 63, 64, 65, 300})
    for (int kind = 0; kind < 5; ++kind)
      for (double a : alphas) {
        std::vector<float> r(n);
        std::vector<int64_t> u(n);
        for (int i = 0; i < n; ++i) {
          const int x = (int)(g() % 41) - 20;
          switch (kind) {
            case 0: r[i] = 0.37f * x; break;
            case 1: r[i] = std::ldexp(1.f, 8 * (x % 9)) * (x < 0 ? -1 : 1); break;  // top bytes
            case 2: r[i] = wh::qsel_float(0x3fc00000u + (uint32_t)(x + 20)); break;  // bottom byte
            case 3: r[i] = wh::qsel_float(0x40000000u + (uint32_t)(x % 3 * 128)); break;  // a boundary
            default: r[i] = x % 2 ? 0.f : (x % 4 ? -0.f : 1e-42f * (x % 3)); break;
          }
          u[i] = kind == 3 ? 1 : g() % 5;
        }
        float want = 0, got = 0;
        const bool hw = brute(r, u, a, &want), hg = select(r, u, a, &got);
        EXPECT(hw == hg);
        if (hw && hg) EXPECT(wh::qsel_bits(want + 0.f) == wh::qsel_bits(got));
      }
  // the lower median of an even unweighted count; zero weights at both ends
  float q = 0;
  EXPECT(select({4.f, 1.f, 3.f, 2.f}, {1, 1, 1, 1}, 0.5, &q) && q == 2.f);
  EXPECT(select({-9.f, 1.f, 2.f, 9.f}, {0, 1, 1, 0}, 0.5, &q) && q == 1.f);
  EXPECT(!select({1.f, 2.f}, {0, 0}, 0.5, &q));
  EXPECT(!select({}, {}, 0.5, &q));
  // bins that do not hold rem: refused, state untouched
  int64_t bins[wh::kQselBins] = {0}, state[2] = {7, 3};
  bins[4] = 2;
  EXPECT(!wh::qsel_pick(bins, 1, 0.5, state) && state[0] == 7 && state[1] == 3);
}

void test_plan() {
  std::vector<int32_t> tasks, red;
  EXPECT(wh::qsel_plan({0, 5, 5, 70}, {5, 5, 70, 200}, 200, 64, &tasks, &red));
  // leaf 0: 1 chunk; leaf 1: empty; leaf 2: 65 rows = 2 chunks; leaf 3: 130 rows = 3 chunks
  EXPECT(tasks.size() == 3 * 6 && red.size() == 3 * 3);
  int64_t covered = 0;
  for (size_t t = 0; t < tasks.size(); t += 3) {
    EXPECT(tasks[t + 1] < tasks[t + 2] && tasks[t + 2] - tasks[t + 1] <= 64);
    covered += tasks[t + 2] - tasks[t + 1];
  }
  EXPECT(covered == 200);
  EXPECT(red[0] == 0 && red[1] == 0 && red[2] == 1);
  EXPECT(red[3] == 2 && red[4] == 1 && red[5] == 2);
  EXPECT(red[6] == 3 && red[7] == 3 && red[8] == 3);
  EXPECT(tasks[3 * 5 + 1] == 198 && tasks[3 * 5 + 2] == 200);
  std::vector<int32_t> t2, r2;
  EXPECT(!wh::qsel_plan({0}, {201}, 200, 64, &t2, &r2));
  EXPECT(!wh::qsel_plan({-1}, {3}, 200, 64, &t2, &r2));
  EXPECT(!wh::qsel_plan({4}, {3}, 200, 64, &t2, &r2));
  EXPECT(!wh::qsel_plan({0}, {3}, 200, 0, &t2, &r2));
  EXPECT(!wh::qsel_plan({0, 1}, {3}, 200, 64, &t2, &r2));
  EXPECT(t2.empty() && r2.empty());
}

}  // namespace

int main() {
  test_key();
  test_weight_threshold();
  test_select();
  test_plan();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
