// The store guard's arithmetic (kv/__init__.py StoreGuard.before_open is the
// Python twin): how many keys / embedding rows the coming open may need, and
// the capacity that holds them. Free of HIP and torch: the native steps
// (csrc/bind/store_guard.h; LinearStep's guard, linear_guard_plan.h, shares
// the table rule) and the host self-test compile the same code.
#pragma once

#include <algorithm>
#include <cstdint>

namespace wh {

// the table rule: past max_load, double until the need fills at most half
inline int64_t grown_cap(int64_t need, int64_t cap, double max_load) {
  if (!((double)need > max_load * (double)cap)) return cap;
  while ((double)need > 0.5 * (double)cap) cap *= 2;
  return cap;
}

// the V slab holds whole rows: double until they fit
inline int64_t grown_vcap(int64_t vneed, int64_t vcap) {
  vcap = std::max<int64_t>(vcap, 1);
  while (vneed > vcap) vcap *= 2;
  return vcap;
}

struct StoreGuardPlan {
  int64_t keys = 0, vused = 0;  // the last summary read
  int64_t since = 0;            // keys opened since the last summary was issued
  // key counts of the last two opens: their pushes may still be in flight
  // and each may allocate one V row per key after the summary
  int64_t recent[2] = {0, 0};

  int64_t need(int64_t n) const { return keys + since + n; }
  int64_t vneed(int64_t n) const { return vused + since + n + recent[0] + recent[1]; }
  void opened(int64_t n) {
    since += n;
    recent[0] = recent[1];
    recent[1] = n;
  }
  void summarised(int64_t k, int64_t v) {
    keys = k;
    vused = v;
    since = 0;
  }
};

}  // namespace wh
