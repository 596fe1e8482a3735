// What the native steps (fm_ops.cc, psx_ops.cc, localize_ahead.h) and the AUC
// chain (auc_ops.cc) share at run time: the native layer's own streams and
// the WH_TIMING=step host timers. Defined in step_rt.cc.
#pragma once
#include "bind_common.h"

#include <array>

namespace wh_bind {

// ---- the native layer's own streams, one per device and role
enum OwnStream { kStreamLinearLs, kStreamPsxLs, kStreamPsxCs, kStreamPsxXs, kStreamAuc, kOwnStreams };
hipStream_t own_stream(int dev, int role);

// ---- WH_TIMING=step: host time per section of a native step
struct HostSplit {
  const char* name;
  double us[10] = {};
  int64_t calls = 0;
  bool abs = false;
  std::vector<std::array<int64_t, 11>> marks;
  explicit HostSplit(const char* n);
  ~HostSplit();
  HostSplit(const HostSplit&) = delete;
  HostSplit& operator=(const HostSplit&) = delete;
  void print() const;
};
class HostTimer {
 public:
  explicit HostTimer(HostSplit* h);
  void mark(int i);
  ~HostTimer();

 private:
  HostSplit* h_;
  std::chrono::steady_clock::time_point t_;
  bool rec_ = false;
  std::array<int64_t, 11> m_{};
};
// a split when WH_TIMING asks for one, else nullptr
HostSplit* host_split(const char* name);
// print every live split now (a short run's summary: the splits print every
// 1000 calls and at their step's destruction, which os._exit skips)
void timing_flush();

}  // namespace wh_bind
