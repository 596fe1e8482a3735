// The native steps' run-time helpers (step_rt.h): their streams and host
// timers.
#include "step_rt.h"

#include <cstdio>
#include <map>
#include <mutex>

namespace wh_bind {

// Streams of the native layer's own (not the c10 pool's round-robin streams,
// one of which RCCL also takes for its internal stream): created once per
// device and role and never destroyed -- the caching allocator records
// events on every stream a block was used on when the block is freed, which
// can be after the step object that used the stream is gone.
hipStream_t own_stream(int dev, int role) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, hipStream_t> m;
  std::lock_guard<std::mutex> lk(mu);
  auto& h = m[{dev, role}];
  if (!h) WH_HIP_CHECK_HOST(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
  return h;
}

// WH_TIMING=step: host time per section of a native step, summed and
// printed (mean us per call) every 1000 calls and at exit -- the launch-
// bound small-minibatch path. WH_TIMING=step2: also the absolute
// steady-clock ns of every mark of calls 200..219 (to line up with a
// rocprofv3 kernel trace).
// Every live split is listed, so that a process leaving through os._exit
// (the bin/ launchers) can still print them: timing_flush()
static std::mutex& split_mu() {
  static std::mutex m;
  return m;
}
static std::vector<HostSplit*>& live_splits() {
  static auto* v = new std::vector<HostSplit*>();
  return *v;
}
HostSplit::HostSplit(const char* n) : name(n) {
  std::lock_guard<std::mutex> lk(split_mu());
  live_splits().push_back(this);
}
HostSplit::~HostSplit() {
  std::lock_guard<std::mutex> lk(split_mu());
  auto& v = live_splits();
  v.erase(std::remove(v.begin(), v.end(), this), v.end());
}
void HostSplit::print() const {
  std::fprintf(stderr, "[%s host us/call over %lld]", name, (long long)calls);
  for (int i = 0; i < 10; ++i)
    if (us[i] > 0) std::fprintf(stderr, " s%d %.2f", i, us[i] / calls);
  std::fprintf(stderr, "\n");
  for (const auto& m : marks) {
    std::fprintf(stderr, "[%s marks ns]", name);
    for (int64_t v : m) std::fprintf(stderr, " %lld", (long long)v);
    std::fprintf(stderr, "\n");
  }
}

static int64_t steady_ns(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(t.time_since_epoch()).count();
}
HostTimer::HostTimer(HostSplit* h) : h_(h) {
  if (h_) {
    t_ = std::chrono::steady_clock::now();
    rec_ = h_->abs && h_->calls >= 200 && h_->calls < 220;
    if (rec_) m_.fill(0), m_[0] = steady_ns(t_);
  }
}
void HostTimer::mark(int i) {
  if (!h_) return;
  const auto n = std::chrono::steady_clock::now();
  h_->us[i] += std::chrono::duration<double, std::micro>(n - t_).count();
  if (rec_ && i + 1 < 11) m_[i + 1] = steady_ns(n);
  t_ = n;
}
HostTimer::~HostTimer() {
  if (!h_) return;
  if (rec_) h_->marks.push_back(m_);
  if (++h_->calls % 1000 == 0) h_->print();
}
void timing_flush() {
  std::lock_guard<std::mutex> lk(split_mu());
  for (const HostSplit* h : live_splits())
    if (h->calls > 0) h->print();
  std::fflush(stderr);
}

HostSplit* host_split(const char* name) {
  const bool abs = timing_on("step2");
  if (!abs && !timing_on("step")) return nullptr;
  auto* h = new HostSplit(name);
  h->abs = abs;
  return h;
}

}  // namespace wh_bind
