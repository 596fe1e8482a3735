// The AUC family (auc, auc_acc, auc_acc_side, auc_join, auc_sorted,
// auc_host_threads): the device chain of csrc/hip/metrics.hip on the current
// stream or on a side stream of the native layer's own, and optionally the
// exact AUC on host threads. The steps (fm_ops.cc, psx_ops.cc) call auc_acc
// and auc_acc_side through ps_ops.h; the chain's persistent workspace is
// dev_ws (hip_ops.cc). Host-only: validates tensors, sizes outputs and
// launches.
#include "ps_ops.h"
#include "step_rt.h"

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>

#include <map>
#include <thread>

#include "host/auc_host.h"
#include "host/auc_jobs.h"

namespace wh_bind {
namespace {

void auc_check(const Tensor& py, const Tensor& label, const Tensor& auc_sum) {
  CHECK_IN(py, torch::kFloat32);
  CHECK_IN(label, torch::kFloat32);
  CHECK_IN(auc_sum, torch::kFloat64);
  TORCH_CHECK(py.numel() == label.numel(), "auc: py/label size mismatch");
  TORCH_CHECK(py.numel() < (int64_t)1 << 30, "auc: at most 2^30 examples per call");
}
// the AUC chain on stream s, which is the current stream (the scratch is its)
void auc_run(const Tensor& py, const Tensor& label, const Tensor& auc_sum, hipStream_t s) {
  const int64_t n = py.numel();
  const int64_t wsb = wh::auc_ws_bytes(n);
  Tensor scratch;
  if (wsb) scratch = torch::empty({wsb}, py.options().dtype(torch::kUInt8));
  wh::auc_accumulate(ptr<float>(py), ptr<float>(label), n, dev_ws(py.device()).auc.data_ptr(),
                     wsb ? scratch.data_ptr() : nullptr, ptr<double>(auc_sum), s);
}

// The chain on a per-device side stream owned here (it waits for the current
// stream first; auc_join makes the current stream wait for it): the Python
// form of this (stream objects, wait_stream, a stream context) cost ~30 us
// of host time per minibatch, which bounds small-minibatch training.
struct AucSide {
  c10::hip::HIPStream s;
  hipEvent_t in, out;
  bool dirty = false;  // AUC work queued on the side stream since the last join
};

AucSide* auc_side(c10::DeviceIndex d, bool create) {
  static std::map<int, AucSide*> m;
  auto it = m.find(d);
  if (it != m.end()) return it->second;
  if (!create) return nullptr;
  // a stream of its own: the pool's round-robin streams are shared (RCCL's
  // internal stream comes from the same pool), and AUC kernels queued on a
  // collective's stream would wait for it
  auto st = c10::hip::getStreamFromExternal(own_stream(d, kStreamAuc), d);
  auto* a = new AucSide{st, nullptr, nullptr};
  WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&a->in, hipEventDisableTiming));
  WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&a->out, hipEventDisableTiming));
  m[d] = a;
  return a;
}

// the stream s waits for the side stream's queued AUC work, if any
void auc_after_side(c10::DeviceIndex d, hipStream_t s) {
  AucSide* a = auc_side(d, false);
  if (!a || !a->dirty) return;
  WH_HIP_CHECK_HOST(hipEventRecord(a->out, a->s.stream()));
  WH_HIP_CHECK_HOST(hipStreamWaitEvent(s, a->out, 0));
  a->dirty = false;
}

// Optionally (WH_AUC_HOST_THREADS=N > 0), a large training minibatch's AUC
// on N host threads: the side stream copies (py, label) into pinned memory
// and a worker computes the exact AUC (csrc/host/auc_host.h: the device
// chain's definition) once the copy's event completes, so the GPU runs no
// AUC kernels. Each job remembers the auc_sum it belongs to; auc_join
// (auc_sum) waits for that tensor's jobs and adds their AUCs, folded in
// submission order (a deterministic sum): the ledger is csrc/host/auc_jobs.h,
// this class its HIP side. Off by default: on the headline step (100k rows)
// it measured level with the device chain (140.0 / 141.9 M vs 140.7 / 139.5 M,
// profiles/round6_p1_isolated.txt), although dropping the AUC altogether
// gains 3-5 % -- the side stream's event pair, the two copies and the join
// remain.
struct HostAuc {
  struct State {
    HostAuc* pool = nullptr;  // never destroyed: os._exit ends the process
    bool on = false;  // new jobs go to the pool (pending ones stay in it after enable(0))
    void enable(int nt) {
      if (nt > 0 && !pool) pool = new HostAuc(nt);
      on = nt > 0;
    }
  };
  // (first use reads the environment: an enable() of that value)
  static State& state() {
    static State s = [] {
      const char* v = std::getenv("WH_AUC_HOST_THREADS");
      State e;
      e.enable(v ? std::atoi(v) : 0);
      return e;
    }();
    return s;
  }

  void submit(const float* py, const float* lab, int64_t n, hipStream_t s, const void* target) {
    wh::AucJob* j = jobs.acquire(n);
    if (!j->cap) {  // a fresh job: its event and pinned buffer
      hipEvent_t ev;
      WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      j->ev = ev;
      const int64_t cap = std::max<int64_t>(n, 1 << 17);
      WH_HIP_CHECK_HOST(hipHostMalloc(reinterpret_cast<void**>(&j->buf), 2 * cap * sizeof(float),
                                      hipHostMallocDefault));
      j->cap = cap;
    }
    WH_HIP_CHECK_HOST(hipMemcpyAsync(j->buf, py, n * sizeof(float), hipMemcpyDeviceToHost, s));
    WH_HIP_CHECK_HOST(hipMemcpyAsync(j->buf + j->cap, lab, n * sizeof(float), hipMemcpyDeviceToHost, s));
    WH_HIP_CHECK_HOST(hipEventRecord(static_cast<hipEvent_t>(j->ev), s));
    jobs.submit(j, target);
  }

  explicit HostAuc(int nt) {
    for (int t = 0; t < nt; ++t) std::thread([this] { run(); }).detach();
  }

  void run() {
    std::vector<uint64_t> ws;
    for (;;) {
      wh::AucJob* j = jobs.take();
      WH_HIP_CHECK_HOST(hipEventSynchronize(static_cast<hipEvent_t>(j->ev)));
      jobs.finish(j, wh::auc_exact_host(j->buf, j->buf + j->cap, j->n, ws));
    }
  }

  wh::AucJobs jobs{64};
};

// The largest minibatch whose AUC runs in order on the current stream: ONE
// launch of a few microseconds (the pairwise k_auc_small), less than the side
// stream's event pair (~4 us of host time in a launch-bound 1000-row step).
// (metrics.hip's kAucSmallMax = 24576 is another decision: the largest
// minibatch the pair kernel takes, on either stream.)
constexpr int64_t kAucOnStreamMax = 4096;

}  // namespace

// auc_sum[0] += exact AUC of (py, label) (sort-free bucketed rank sum)
void auc_acc(const Tensor& py, const Tensor& label, const Tensor& auc_sum) {
  auc_check(py, label, auc_sum);
  c10::DeviceGuard g(py.device());
  auc_after_side(py.device().index(), cur_stream(py));  // (the workspace is shared)
  auc_run(py, label, auc_sum, cur_stream(py));
}

void auc_acc_side(const Tensor& py, const Tensor& label, const Tensor& auc_sum) {
  auc_check(py, label, auc_sum);
  if (py.numel() <= kAucOnStreamMax) return auc_acc(py, label, auc_sum);
  c10::DeviceGuard g(py.device());
  AucSide* a = auc_side(py.device().index(), true);
  WH_HIP_CHECK_HOST(hipEventRecord(a->in, cur_stream(py)));
  WH_HIP_CHECK_HOST(hipStreamWaitEvent(a->s.stream(), a->in, 0));
  c10::hip::HIPCachingAllocator::recordStream(py.storage().data_ptr(), a->s);
  c10::hip::HIPCachingAllocator::recordStream(label.storage().data_ptr(), a->s);
  if (HostAuc::state().on) {  // (the copies touch no shared workspace: not dirty)
    HostAuc::state().pool->submit(ptr<float>(py), ptr<float>(label), py.numel(), a->s.stream(),
                                  auc_sum.data_ptr());
    return;
  }
  a->dirty = true;
  c10::hip::HIPStreamGuard sg(a->s);  // the scratch is the side stream's
  auc_run(py, label, auc_sum, a->s.stream());
}

static void auc_join(const Tensor& auc_sum) {
  if (!auc_sum.is_cuda()) return;
  c10::DeviceGuard g(auc_sum.device());
  auc_after_side(auc_sum.device().index(), cur_stream(auc_sum));
  double s;  // its host-thread jobs, if any: their AUCs summed in submission order
  HostAuc* h = HostAuc::state().pool;
  if (h && h->jobs.join(auc_sum.data_ptr(), &s)) auc_sum.add_(s);
}

static Tensor auc(const Tensor& py, const Tensor& label) {
  auto out = torch::zeros({1}, py.options().dtype(torch::kFloat64));
  auc_acc(py, label, out);
  return out;
}

// reference path: rocPRIM radix sort + rank-sum (kept as a cross-check)
static Tensor auc_sorted(const Tensor& py, const Tensor& label) {
  CHECK_IN(py, torch::kFloat32);
  CHECK_IN(label, torch::kFloat32);
  c10::DeviceGuard g(py.device());
  const int64_t n = py.numel();
  auto pys = torch::empty_like(py);
  auto lab = torch::empty_like(label);
  const size_t sbytes = wh::auc_sort_tmp_bytes(n);
  auto stmp = torch::empty({(int64_t)sbytes + 16}, py.options().dtype(torch::kUInt8));
  wh::sort_by_score(ptr<float>(py), ptr<float>(label), n, ptr<float>(pys), ptr<float>(lab),
                    stmp.data_ptr(), sbytes, cur_stream(py));
  auto tmp = torch::empty({n / 2 + 1 + n + 1 + wh::scan_tmp_elems(n)},
                          py.options().dtype(torch::kInt64));
  auto out = torch::empty({2}, py.options().dtype(torch::kFloat64));
  wh::auc_from_sorted(ptr<float>(lab), n, ptr<double>(out), ptr<int64_t>(tmp), cur_stream(py));
  return out.narrow(0, 0, 1);
}

void bind_auc(py::module_& m) {
  m.def("auc", &auc);
  m.def("auc_acc", &auc_acc);
  m.def("auc_acc_side", &auc_acc_side);
  m.def("auc_join", &auc_join);
  m.def("auc_host_threads", [](int n) { HostAuc::state().enable(n); },
        "large training minibatches' AUC on n host threads (0: the device chain)");
  m.def("auc_sorted", &auc_sorted);
}

}  // namespace wh_bind
