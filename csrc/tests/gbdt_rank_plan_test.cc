// Stand-alone test of the ranking task plan (csrc/host/gbdt_rank_plan.h): no
// torch, no HIP. build_native.py builds it plain (bin/native/) and under
// -fsanitize=address,undefined (--sanitize-rank-plan); exit status 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <set>

#include "host/gbdt_rank_plan.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

std::vector<int64_t> offsets(const std::vector<int64_t>& sizes) {
  std::vector<int64_t> off(1, 0);
  for (int64_t s : sizes) off.push_back(off.back() + s);
  return off;
}

bool throws(const std::vector<int64_t>& off, int64_t n) {
  try {
    wh::gbdt_rank_plan(off.data(), off.size(), n);
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

// every non-empty group once, in its class, larger groups first
void check(const std::vector<int64_t>& sizes, int64_t lds_rows) {
  const auto off = offsets(sizes);
  const auto p = wh::gbdt_rank_plan(off.data(), off.size(), off.back(), lds_rows);
  std::set<int32_t> seen;
  const std::vector<int32_t>* lists[3] = {&p.small, &p.block, &p.tiled};
  for (int c = 0; c < 3; ++c) {
    int64_t prev = INT64_MAX;
    for (int32_t g : *lists[c]) {
      EXPECT(g >= 0 && (size_t)g < sizes.size());
      const int64_t len = sizes[g];
      EXPECT(seen.insert(g).second);
      EXPECT(len > 0 && len <= prev);
      prev = len;
      const int cls = len <= wh::kRankWaveRows ? 0 : len <= lds_rows ? 1 : 2;
      EXPECT(cls == c);
    }
  }
  size_t nonempty = 0;
  for (int64_t s : sizes) nonempty += s > 0;
  EXPECT(seen.size() == nonempty);
  EXPECT(p.max_block_rows == (p.block.empty() ? 0 : sizes[p.block[0]]));
  EXPECT(p.max_tiled_rows == (p.tiled.empty() ? 0 : sizes[p.tiled[0]]));
}

}  // namespace

int main() {
  const int64_t C = wh::gbdt_rank_lds_rows();
  EXPECT(C >= wh::kRankWaveRows && C * 16 <= 160 * 1024);
  check({0, 1, 2, 64, 65, C, C + 1, 0, 3}, C);
  check({}, C);
  check({0, 0, 0}, C);
  check({5}, C);
  check({100, 300, 200, 64, 128}, 128);
  std::mt19937 rng(7);
  for (int rep = 0; rep < 20; ++rep) {
    std::vector<int64_t> sizes(1 + rng() % 500);
    for (auto& s : sizes) s = rng() % 4 == 0 ? 0 : (int64_t)(rng() % (3 * C));
    check(sizes, C);
  }
  {  // ties keep the lower id first
    const auto off = offsets({3, 7, 3, 7});
    const auto p = wh::gbdt_rank_plan(off.data(), off.size(), 20);
    EXPECT((p.small == std::vector<int32_t>{1, 3, 0, 2}));
  }
  // malformed: empty input, a first offset other than 0, a decrease, a last
  // offset other than n, n above INT32_MAX
  EXPECT(throws({}, 0));
  EXPECT(throws({1, 3}, 3));
  EXPECT(throws({0, 4, 2, 6}, 6));
  EXPECT(throws({0, 2, 5}, 6));
  EXPECT(throws({0, (int64_t)INT32_MAX + 1}, (int64_t)INT32_MAX + 1));
  EXPECT(!throws({0}, 0));
  EXPECT(!throws({0, (int64_t)INT32_MAX}, INT32_MAX));
  if (failures) {
    std::fprintf(stderr, "gbdt_rank_plan_test: %d failure(s)\n", failures);
    return 1;
  }
  std::puts("gbdt_rank_plan_test ok");
  return 0;
}
