// Stand-alone test of the survival objectives' host parts
// (csrc/host/gbdt_survival_plan.h, csrc/host/gbdt_aft.h): no torch, no HIP.
// build_native.py builds it plain (bin/native/) and under
// -fsanitize=address,undefined (--sanitize-survival-plan); exit status 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "host/gbdt_aft.h"
#include "host/gbdt_survival_plan.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

void test_tiles() {
  const int64_t T = wh::gbdt_cox_tile();
  EXPECT(T == wh::kCoxThreads * wh::kCoxItems);
  EXPECT(wh::gbdt_cox_tiles(0) == 0 && wh::gbdt_cox_tiles(-3) == 0);
  EXPECT(wh::gbdt_cox_tiles(1) == 1 && wh::gbdt_cox_tiles(T - 1) == 1);
  EXPECT(wh::gbdt_cox_tiles(T) == 1 && wh::gbdt_cox_tiles(T + 1) == 2);
  EXPECT(wh::gbdt_cox_tiles(3 * T + 5) == 4);
  EXPECT(wh::gbdt_cox_tiles(((int64_t)1 << 31) - 1) == (((int64_t)1 << 31) - 1 + T - 1) / T);
  for (int64_t n : {(int64_t)0, (int64_t)1, T, T + 1, 3 * T + 5}) {
    const wh::CoxWs w = wh::gbdt_cox_ws(n);
    const int64_t nt = wh::gbdt_cox_tiles(n);
    // the parts follow each other without overlap
    EXPECT(w.mstar == 0 && w.e == 1 && w.S == w.e + n && w.part == w.S + n);
    EXPECT(w.off == w.part + 4 * nt && w.off2 == w.off + nt && w.size == w.off2 + 2 * nt);
  }
}

void test_runs() {
  // times 1 1 | 2 | 3 3 3 | 5, events marked
  const std::vector<float> t = {1, 1, 2, 3, 3, 3, 5};
  const std::vector<uint8_t> d = {0, 1, 1, 1, 1, 0, 0};
  const int64_t n = (int64_t)t.size();
  std::vector<int32_t> head(n), tail(n), ev(n);
  EXPECT(wh::gbdt_cox_runs(t.data(), d.data(), n, head.data(), tail.data(), ev.data()) == 4);
  const std::vector<int32_t> eh = {0, 0, 2, 3, 3, 3, 6}, et = {1, 1, 2, 5, 5, 5, 6},
                             ee = {1, 0, 1, 2, 0, 0, 0};
  EXPECT(head == eh && tail == et && ev == ee);
  // all rows tied; no rows; one row
  std::vector<float> same(5, 2.5f);
  std::vector<uint8_t> all(5, 1);
  head.assign(5, -1), tail.assign(5, -1), ev.assign(5, -1);
  EXPECT(wh::gbdt_cox_runs(same.data(), all.data(), 5, head.data(), tail.data(), ev.data()) == 5);
  for (int i = 0; i < 5; ++i) EXPECT(head[i] == 0 && tail[i] == 4 && ev[i] == (i ? 0 : 5));
  EXPECT(wh::gbdt_cox_runs(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == 0);
  EXPECT(wh::gbdt_cox_runs(same.data(), all.data(), 1, head.data(), tail.data(), ev.data()) == 1);
  EXPECT(head[0] == 0 && tail[0] == 0 && ev[0] == 1);
  // a NaN time is a run of its own: the loop ends
  const std::vector<float> tn = {1, NAN, NAN, 2};
  const std::vector<uint8_t> dn = {1, 1, 0, 1};
  head.assign(4, -1), tail.assign(4, -1), ev.assign(4, -1);
  EXPECT(wh::gbdt_cox_runs(tn.data(), dn.data(), 4, head.data(), tail.data(), ev.data()) == 3);
  for (int i = 0; i < 4; ++i) EXPECT(head[i] == i && tail[i] == i && ev[i] == dn[i]);
  // a run across a tile boundary: heads and tails do not stop at it
  const int64_t T = wh::gbdt_cox_tile(), m = T + 8;
  std::vector<float> tt(m);
  std::vector<uint8_t> dd(m, 1);
  for (int64_t i = 0; i < m; ++i) tt[i] = i >= T - 3 && i <= T + 3 ? (float)(T - 3) : (float)i;
  head.assign(m, -1), tail.assign(m, -1), ev.assign(m, -1);
  EXPECT(wh::gbdt_cox_runs(tt.data(), dd.data(), m, head.data(), tail.data(), ev.data()) == m);
  for (int64_t i = T - 3; i <= T + 3; ++i)
    EXPECT(head[i] == T - 3 && tail[i] == T + 3 && ev[i] == (i == T - 3 ? 7 : 0));
  EXPECT(head[T - 4] == T - 4 && tail[T - 4] == T - 4 && head[T + 4] == T + 4);
}

template <int DIST>
void check_pair(double m, double yl, double yu, double sigma) {
  // the pair against central differences of the fp64 loss (where the
  // likelihood is above the metric's floor and the pair inside the clamps)
  const double d = 1e-3;
  const double l0 = wh::gbdt_aft_loss(DIST, m, yl, yu, sigma);
  const double lp = wh::gbdt_aft_loss(DIST, m + d, yl, yu, sigma);
  const double lm = wh::gbdt_aft_loss(DIST, m - d, yl, yu, sigma);
  const double g = (lp - lm) / (2 * d), h = (lp - 2 * l0 + lm) / (d * d);
  const wh::GbdtPair p = wh::gbdt_aft_pair<DIST>((float)m, (float)yl, (float)yu, (float)sigma);
  EXPECT(std::isfinite(p.g) && std::isfinite(p.h));
  if (l0 < 20 && std::fabs(g) < 14 && h > 1e-3 && h < 14) {
    EXPECT(std::fabs(p.g - g) <= 1e-3 * (1 + std::fabs(g)));
    EXPECT(std::fabs(p.h - h) <= 1e-2 * (1 + std::fabs(h)));
  }
}

template <int DIST>
void test_aft_dist() {
  const double inf = std::numeric_limits<double>::infinity();
  for (double sigma : {0.5, 1.0, 2.0})
    for (double m : {-2.0, -0.5, 0.0, 0.7, 2.5})
      for (double y : {0.3, 1.0, 4.0}) {
        check_pair<DIST>(m, y, y, sigma);
        check_pair<DIST>(m, y, inf, sigma);
        check_pair<DIST>(m, 0.0, y, sigma);
        check_pair<DIST>(m, y, 2.5 * y, sigma);
      }
  // the tails: finite, inside xgboost's clamps, at them where z runs off
  for (float z : {-40.f, -12.f, 12.f, 40.f, 200.f, -200.f}) {
    const float y = 2.f, m = std::log(y) - z;
    const float bounds[4][2] = {{y, y}, {y, INFINITY}, {0.f, y}, {y, 3.f * y}};
    for (const auto& b : bounds) {
      const wh::GbdtPair p = wh::gbdt_aft_pair<DIST>(m, b[0], b[1], 1.f);
      EXPECT(std::isfinite(p.g) && std::isfinite(p.h));
      EXPECT(p.g >= wh::kAftMinG && p.g <= wh::kAftMaxG);
      EXPECT(p.h >= (float)wh::kAftMinH && p.h <= wh::kAftMaxH);
      EXPECT(std::isfinite(wh::gbdt_aft_loss(DIST, m, b[0], b[1], 1.0)));
    }
  }
  // a right-censored row far above its bound carries no information ...
  wh::GbdtPair p = wh::gbdt_aft_pair<DIST>(40.f, 1.f, INFINITY, 1.f);
  EXPECT(std::fabs(p.g) < 1e-6f && p.h <= 1e-6f);
  // ... one far below is pushed up (to the clamp where the law's pull grows with z)
  p = wh::gbdt_aft_pair<DIST>(-40.f, 1.f, INFINITY, 1.f);
  EXPECT(DIST == wh::kAftLogistic ? std::fabs(p.g + 1.f) < 1e-6f : p.g == wh::kAftMinG);
  // ... and a left-censored row far above its bound is pushed down
  p = wh::gbdt_aft_pair<DIST>(40.f, 0.f, 1.f, 1.f);
  EXPECT(DIST == wh::kAftNormal ? p.g == wh::kAftMaxG : std::fabs(p.g - 1.f) < 1e-6f);
}

void test_aft() {
  test_aft_dist<wh::kAftNormal>();
  test_aft_dist<wh::kAftLogistic>();
  test_aft_dist<wh::kAftExtreme>();
  // uncensored closed forms
  wh::GbdtPair p = wh::gbdt_aft_pair<wh::kAftNormal>(0.f, std::exp(1.5f), std::exp(1.5f), 2.f);
  EXPECT(std::fabs(p.g - (-0.75f / 2.f)) < 1e-6f && std::fabs(p.h - 0.25f) < 1e-7f);
  p = wh::gbdt_aft_pair<wh::kAftLogistic>(0.f, 1.f, 1.f, 1.f);
  EXPECT(std::fabs(p.g) < 1e-7f && std::fabs(p.h - 0.5f) < 1e-7f);
  p = wh::gbdt_aft_pair<wh::kAftExtreme>(0.f, 1.f, 1.f, 1.f);
  EXPECT(std::fabs(p.g) < 1e-7f && std::fabs(p.h - 1.f) < 1e-7f);
  // the Mills ratio joins its series smoothly and vanishes at inf
  EXPECT(std::fabs(wh::aft_erfcx(25.0 - 1e-9) / wh::aft_erfcx(25.0) - 1.0) < 1e-7);
  EXPECT(std::fabs(wh::aft_mills(0.f) - 1.2533141f) < 1e-6f);
  EXPECT(wh::aft_mills(INFINITY) == 0.f);
}

}  // namespace

int main() {
  test_tiles();
  test_runs();
  test_aft();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
