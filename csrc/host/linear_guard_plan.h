// The arithmetic of LinearStep's store guard (csrc/bind/fm_ops.cc): a guard
// that never waits per step. Table summaries are read whenever they have
// landed; in between, the key count is bounded by the last count read plus
// the ids issued since that summary was stamped. Free of HIP and torch: the
// step and the host self-test compile the same code. (The other native
// steps' guard, one summary per open, is store_guard_plan.h; the table's
// growth rule, grown_cap, is shared.)
#pragma once

#include <cstdint>

#include "host/store_guard_plan.h"

namespace wh {

struct LinearGuardPlan {
  // A summary (a kernel and a 32-byte read-back on the compute stream) every
  // kGuardEvery steps, or every step once the bound nears the load limit:
  // between summaries the bound grows by the inserts issued, so a late
  // summary only makes the grow decision more conservative, and a failed
  // insert still stops training within kGuardEvery steps (and at the flush).
  static constexpr int kGuardEvery = 8;

  int64_t issued = 0;       // ids handed to find-or-insert so far
  int64_t base_keys = 0;    // the key count of the newest summary read ...
  int64_t base_issued = 0;  // ... and the `issued` it was stamped with
  int64_t step = 0;         // unforced calls of due()

  // at most this many keys are in the table
  int64_t bound() const { return base_keys + (issued - base_issued); }
  // the capacity that holds an open of n ids, every one of them new
  int64_t grow_target(int64_t n, int64_t cap, double max_load) const {
    return grown_cap(bound() + n, cap, max_load);
  }
  // n ids were issued: is a summary due now? (A forced call does not advance
  // the cadence.)
  bool due(int64_t n, int64_t cap, double max_load, bool force) {
    issued += n;
    if (force || ++step % kGuardEvery == 0) return true;
    return !((double)bound() + (double)n * kGuardEvery < 0.9 * (max_load * (double)cap));
  }
  // A summary read: `keys` in the table when `stamped` ids had been issued.
  // Summaries are read as they land, so one older than the base is dropped.
  void summarised(int64_t keys, int64_t stamped) {
    if (stamped < base_issued) return;
    base_keys = keys;
    base_issued = stamped;
  }
};

}  // namespace wh
