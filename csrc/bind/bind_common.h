// What every translation unit of the binding layer (module wormhole_amd._hip)
// needs: the torch / pybind11 / HIP includes, the tensor checks and the
// stateless helpers, and one registration function per op family. State
// (device workspaces, the deterministic / timing switches, the KVStore)
// lives in hip_ops.cc only.
#pragma once
#include <torch/extension.h>
#include <pybind11/stl.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
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

template <typename T>
const T* optptr(const c10::optional<Tensor>& t) {
  return (t.has_value() && t->defined() && t->numel() > 0) ? reinterpret_cast<const T*>(t->data_ptr())
                                                           : nullptr;
}

inline int64_t next_pow2(int64_t x) {
  int64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

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

// A ring of pinned staging buffers for stream-ordered uploads: a slot is
// rewritten only after the copy that last read it has run (its event), so
// the host never has to drain the stream to reuse staging memory.
class PinnedRing {
 public:
  static constexpr int N = 4;
  ~PinnedRing() {
    for (auto& e : ev_)
      if (e) (void)hipEventDestroy(e);
  }
  template <typename T>
  T* get(int64_t n) {
    cur_ = (cur_ + 1) % N;
    if (ev_[cur_]) WH_HIP_CHECK_HOST(hipEventSynchronize(ev_[cur_]));
    return buf_[cur_].get<T>(n);
  }
  Tensor tensor() const { return buf_[cur_].tensor(); }
  // after enqueuing the copy that reads the current slot
  void mark(hipStream_t s) {
    if (!ev_[cur_]) WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&ev_[cur_], hipEventDisableTiming));
    WH_HIP_CHECK_HOST(hipEventRecord(ev_[cur_], s));
  }

 private:
  PinnedBuf buf_[N];
  hipEvent_t ev_[N] = {nullptr, nullptr, nullptr, nullptr};
  int cur_ = N - 1;
};

// each family's m.def calls (defined in <family>_ops.cc, called by
// PYBIND11_MODULE in hip_ops.cc)
void bind_gbdt(py::module_& m);
void bind_kmeans(py::module_& m);
void bind_bsp(py::module_& m);
void bind_ingest(py::module_& m);

}  // namespace wh_bind
