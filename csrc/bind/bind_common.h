// What every translation unit of the binding layer (module wormhole_amd._hip)
// needs: the torch / pybind11 / HIP includes, the tensor checks and the
// stateless helpers, the process-wide switches (deterministic, timing) and
// one registration function per op family. State lives with its owner: the
// localize workspace in localize_ops.cc, every other device workspace in
// hip_ops.cc (DevWs, declared in ps_ops.h for fm_ops.cc and auc_ops.cc), the
// AUC side stream and host-thread pool in auc_ops.cc, the native layer's own
// streams and host timers in step_rt.cc; the KVStore is kv_store.h.
#pragma once
#include <torch/extension.h>
#include <pybind11/stl.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "hip/wh_kernels.h"

namespace py = pybind11;

#define CHECK_DEV(t) TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor")
#define CHECK_CONT(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHECK_DT(t, dt) TORCH_CHECK((t).scalar_type() == (dt), #t " has wrong dtype ", (t).scalar_type())
#define CHECK_IN(t, dt) \
  CHECK_DEV(t);         \
  CHECK_CONT(t);        \
  CHECK_DT(t, dt)

#define WH_HIP_CHECK_HOST(expr)                                                   \
  do {                                                                          \
    hipError_t _e = (expr);                                                     \
    TORCH_CHECK(_e == hipSuccess, "HIP error ", hipGetErrorString(_e), " at ",  \
                __FILE__, ":", __LINE__);                                       \
  } while (0)

namespace wh_bind {

using torch::Tensor;

inline hipStream_t cur_stream(const Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

template <typename T>
T* ptr(const Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }

// an optional tensor that is really there: given, defined and non-empty
inline bool present(const c10::optional<Tensor>& t) {
  return t.has_value() && t->defined() && t->numel() > 0;
}

template <typename T>
const T* optptr(const c10::optional<Tensor>& t) {
  return present(t) ? reinterpret_cast<const T*>(t->data_ptr()) : nullptr;
}

inline int64_t next_pow2(int64_t x) {
  int64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// Sub-buffers of ONE allocation (separate tensors are separate trips through
// the allocator and dispatcher, host time of the launch-bound steps): add()
// every piece, alloc() the uint8 block, then take typed views, which keep the
// block alive as long as any of them is in use, or raw pointers. Pieces start
// on 256-byte boundaries.
class Carve {
 public:
  int64_t add(int64_t bytes) {
    const int64_t o = at_;
    at_ += (bytes + 255) / 256 * 256;
    return o;
  }
  void alloc(const torch::TensorOptions& like) {
    blk_ = torch::empty({std::max<int64_t>(at_, 256)}, like.dtype(torch::kUInt8));
  }
  Tensor view(int64_t off, int64_t n, torch::ScalarType dt) const {
    return blk_.narrow(0, off, n * (int64_t)c10::elementSize(dt)).view(dt);
  }
  template <typename T>
  T* at(int64_t off) const { return reinterpret_cast<T*>(static_cast<char*>(blk_.data_ptr()) + off); }

 private:
  int64_t at_ = 0;
  Tensor blk_;
};

class PinnedBuf {
 public:
  template <typename T>
  T* get(int64_t n) {
    const int64_t bytes = std::max<int64_t>(n * (int64_t)sizeof(T), 8);
    if (!t_.defined() || t_.numel() < bytes)
      t_ = torch::empty({bytes * 2}, torch::TensorOptions().dtype(torch::kUInt8).pinned_memory(true));
    return reinterpret_cast<T*>(t_.data_ptr());
  }
  Tensor tensor() const { return t_; }

 private:
  Tensor t_;
};

// A HIP event that dies with its holder. Default-constructed it is empty: a
// holder creates its events in its constructor's body, under its device
// guard. Holders whose destructor synchronises the device keep their events
// as members, which are destroyed after the destructor's body.
class Event {
 public:
  Event() = default;
  explicit Event(bool timing) { create(timing); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  void create(bool timing = false) {
    TORCH_CHECK(!e_, "Event: created twice");
    WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&e_, timing ? hipEventDefault : hipEventDisableTiming));
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

// A ring of N pinned staging buffers for stream-ordered uploads: a slot is
// rewritten only after the copy that last read it has run (its event), so
// the host never has to drain the stream to reuse staging memory.
template <int N>
class PinnedRing {
 public:
  // the next get() waits for the copy that last read its slot
  bool next_used() const { return ev_[(cur_ + 1) % N] != nullptr; }
  template <typename T>
  T* get(int64_t n) {
    cur_ = (cur_ + 1) % N;
    if (ev_[cur_]) WH_HIP_CHECK_HOST(hipEventSynchronize(ev_[cur_]));
    return buf_[cur_].template get<T>(n);
  }
  Tensor tensor() const { return buf_[cur_].tensor(); }
  // after enqueuing the copy that reads the current slot
  void mark(hipStream_t s) {
    if (!ev_[cur_]) ev_[cur_].create();
    WH_HIP_CHECK_HOST(hipEventRecord(ev_[cur_], s));
  }

 private:
  PinnedBuf buf_[N];
  Event ev_[N];
  int cur_ = N - 1;
};

// The host's wait for a step's one device read (the localize counts, the
// store guard's summary): polled for up to 2 ms before a blocking wait. The
// step's next launches go out the moment the read lands instead of after a
// sleeping wait's wake-up (A/B on one box: headline 142.8-143.4 vs
// 140.9-143.5 M, loopback 8 123.8 / 125.7 vs 123.2 / 125.1 M; within noise
// elsewhere: profiles/round6_small_minibatch_host.txt).
inline void wait_event(hipEvent_t e) {
#if !defined(WH_BLOCKING_WAIT)
  const auto t0 = std::chrono::steady_clock::now();
  while (true) {
    const hipError_t r = hipEventQuery(e);
    if (r == hipSuccess) return;
    WH_HIP_CHECK_HOST(r == hipErrorNotReady ? hipSuccess : r);
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
  }
#endif
  WH_HIP_CHECK_HOST(hipEventSynchronize(e));
}

// WH_DETERMINISTIC=1: bitwise-repeatable training steps: the
// hash + stable-sort localize and ordered (atomic-free) gradient reductions
inline bool deterministic() {
  static int on = -1;
  if (on < 0) {
    const char* d = std::getenv("WH_DETERMINISTIC");
    on = d && std::string(d) == "1";
  }
  return on == 1;
}

// WH_TIMING: comma-separated profiling aids (docs/build.md): step, step2,
// loc, ingest, comm. True when `what` is one of the listed items.
inline bool timing_on(const char* what) {
  const char* e = std::getenv("WH_TIMING");
  if (!e) return false;
  const std::string v = std::string(",") + e + ",";
  return v.find(std::string(",") + what + ",") != std::string::npos;
}

// each family's m.def calls (defined in <family>_ops.cc, called by
// PYBIND11_MODULE in hip_ops.cc)
void bind_gbdt(py::module_& m);
void bind_kmeans(py::module_& m);
void bind_bsp(py::module_& m);
void bind_ingest(py::module_& m);
void bind_localize(py::module_& m);
void bind_fm(py::module_& m);
void bind_psx(py::module_& m);
void bind_auc(py::module_& m);

}  // namespace wh_bind
