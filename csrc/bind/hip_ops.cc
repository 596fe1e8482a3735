// torch / pybind11 binding layer for the gfx950 HIP kernels (module
// wormhole_amd._hip): the module itself and everything that shares the
// parameter-server state -- the device workspaces, KVStore's bindings (the
// class is kv_store.h), the ps_* ops of the multi-shard exchange, the native
// layer's streams and host timers, the AUC chain, quantisation. FM and the
// single-shard native steps (fm_ops.cc), the multi-shard step and RCCL
// (psx_ops.cc), localize (localize_ops.cc) and the stateless BSP families
// (gbdt_ops.cc, kmeans_ops.cc, bsp_ops.cc, ingest_ops.cc) have translation
// units of their own, registered from PYBIND11_MODULE below; what those call
// here is declared in ps_ops.h. Host-only: validates tensors, sizes outputs
// and launches on the current PyTorch HIP stream.
#include "bind_common.h"
#include "kv_store.h"
#include "ps_ops.h"

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPCachingAllocator.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <deque>
#include <map>
#include <mutex>
#include <condition_variable>
#include <thread>
#include <string>
#include <vector>

#include "host/auc_host.h"

using namespace wh_bind;

// (in wh_bind, not an anonymous namespace: fm_ops.cc and psx_ops.cc call some
// of these)
namespace wh_bind {

DevWs& dev_ws(const torch::Device& d) {
  static std::vector<DevWs*> ws(64, nullptr);
  const int i = d.index() < 0 ? 0 : d.index();
  TORCH_CHECK(i < 64, "device index out of range");
  if (!ws[i]) {
    auto o = torch::TensorOptions().device(d);
    auto* w = new DevWs();
    w->lb = torch::zeros({wh::lookback_ws_words()}, o.dtype(torch::kInt64));
    w->auc = torch::zeros({wh::auc_ws_persistent_bytes() / 8}, o.dtype(torch::kInt64));
    w->auc.select(0, wh::auc_ws_lohi_offset() / 8).fill_(-1);
    w->fwd_ticket = torch::zeros({wh::fwd_ticket_words()}, o.dtype(torch::kInt32));
    ws[i] = w;
  }
  return *ws[i];
}

wh::Lookback lookback(const torch::Device& d) {
  return wh::lookback_bind(dev_ws(d).lb.data_ptr());
}

// ------------------------------------------------------------------ scan
Tensor scan_excl(const Tensor& in) {
  CHECK_DEV(in); CHECK_CONT(in);
  c10::DeviceGuard g(in.device());
  const int64_t n = in.numel();
  auto o = torch::empty({n + 1}, in.options().dtype(torch::kInt64));
  auto tmp = torch::empty({wh::scan_tmp_elems(n)}, in.options().dtype(torch::kInt64));
  if (in.scalar_type() == torch::kInt32)
    wh::scan_i32(ptr<int32_t>(in), ptr<int64_t>(o), n, ptr<int64_t>(tmp), cur_stream(in));
  else {
    CHECK_DT(in, torch::kInt64);
    wh::scan_i64(ptr<int64_t>(in), ptr<int64_t>(o), n, ptr<int64_t>(tmp), cur_stream(in));
  }
  return o;
}

// worker side of the multi-shard exchange (psx.hip). rbuf: the received pull
// reply [R, vstride]; segS/segHS: int64 [P+1] over the keys sent per owner;
// vrecv: int64 [P] V rows received per owner. Returns (hdr [U, 2], rows
// int64 [1] = R actually used).
std::vector<Tensor> ps_unpack(const Tensor& rbuf, int64_t U, const Tensor& segS,
                              const Tensor& segHS, const Tensor& vrecv) {
  CHECK_IN(rbuf, torch::kFloat32);
  CHECK_IN(segS, torch::kInt64);
  CHECK_IN(segHS, torch::kInt64);
  CHECK_IN(vrecv, torch::kInt64);
  TORCH_CHECK(rbuf.dim() == 2, "ps_unpack: rbuf must be [R, vstride]");
  const int P = (int)segS.numel() - 1;
  TORCH_CHECK(segHS.numel() == P + 1 && vrecv.numel() == P, "ps_unpack: bad segment tables");
  c10::DeviceGuard g(rbuf.device());
  auto hdr = torch::empty({U, 2}, rbuf.options());
  auto rows = torch::empty({1}, segS.options());
  TORCH_CHECK(wh::ps_unpack(ptr<float>(rbuf), U, (int)rbuf.size(1), ptr<int64_t>(segS),
                            ptr<int64_t>(segHS), ptr<int64_t>(vrecv), P, ptr<float>(hdr),
                            ptr<int64_t>(rows), cur_stream(rbuf)),
              "ps_unpack: limits exceeded");
  return {hdr, rows};
}

// 12-byte key records {lo, hi, count} int32 [U, 3] (ucnt optional)
Tensor ps_records(const Tensor& uniq, const c10::optional<Tensor>& ucnt) {
  CHECK_IN(uniq, torch::kInt64);
  const int32_t* cp = nullptr;
  if (ucnt.has_value() && ucnt->defined()) {
    CHECK_IN((*ucnt), torch::kInt32);
    TORCH_CHECK(ucnt->numel() == uniq.numel(), "ps_records: count size mismatch");
    cp = ptr<int32_t>(*ucnt);
  }
  c10::DeviceGuard g(uniq.device());
  auto rec = torch::empty({uniq.numel(), 3}, uniq.options().dtype(torch::kInt32));
  wh::ps_records(reinterpret_cast<const uint64_t*>(uniq.data_ptr()), cp, uniq.numel(),
                 ptr<int32_t>(rec), cur_stream(uniq));
  return rec;
}

// C0 buffers from the owner counts [S+1] (S shards + the overflow flag), the
// V row counts [P] (optional) and this rank's has-data flag: (send int64
// [4P], payload int64 [S+1+5P]; payload[S+1 : S+1+4P] is the exchange's
// receive slot)
std::vector<Tensor> ps_c0(const Tensor& owner_cnt, const c10::optional<Tensor>& vcnt, int64_t P,
                          int64_t flag, bool loopback) {
  CHECK_IN(owner_cnt, torch::kInt64);
  const int S = (int)owner_cnt.numel() - 1;
  TORCH_CHECK(S >= 1 && S <= P, "ps_c0: owner counts must cover 1..P shards");
  const int64_t* vp = nullptr;
  if (vcnt.has_value() && vcnt->defined()) {
    CHECK_IN((*vcnt), torch::kInt64);
    TORCH_CHECK(vcnt->numel() == P, "ps_c0: vcnt size mismatch");
    vp = ptr<int64_t>(*vcnt);
  }
  c10::DeviceGuard g(owner_cnt.device());
  auto send = torch::empty({4 * P}, owner_cnt.options());
  auto payload = torch::empty({S + 1 + 5 * P}, owner_cnt.options());
  TORCH_CHECK(wh::ps_c0(ptr<int64_t>(owner_cnt), vp, S, (int)P, flag, ptr<int64_t>(send),
                        ptr<int64_t>(payload), cur_stream(owner_cnt), loopback ? 1 : 0),
              "ps_c0: too many peers");
  return {send, payload};
}

// gw [U] into the header rows of the push buffer gbuf [R, vstride] (in place)
void ps_pack_gw(const Tensor& gw, const Tensor& gbuf, const Tensor& segS, const Tensor& segHS,
                const Tensor& vrecv) {
  CHECK_IN(gw, torch::kFloat32);
  CHECK_IN(gbuf, torch::kFloat32);
  CHECK_IN(segS, torch::kInt64);
  CHECK_IN(segHS, torch::kInt64);
  CHECK_IN(vrecv, torch::kInt64);
  TORCH_CHECK(gbuf.dim() == 2, "ps_pack_gw: gbuf must be [R, vstride]");
  const int P = (int)segS.numel() - 1;
  c10::DeviceGuard g(gw.device());
  TORCH_CHECK(wh::ps_pack_gw(ptr<float>(gw), gw.numel(), (int)gbuf.size(1), ptr<int64_t>(segS),
                             ptr<int64_t>(segHS), ptr<int64_t>(vrecv), P, ptr<float>(gbuf),
                             cur_stream(gw)),
              "ps_pack_gw: limits exceeded");
}

// worker side of a multi-shard pull: renumber hdr vidx into local compact
// order; returns m as a device int64 [1] tensor
Tensor vidx_renumber(const Tensor& hdr) {
  CHECK_IN(hdr, torch::kFloat32);
  c10::DeviceGuard g(hdr.device());
  const int64_t n = hdr.numel() / 2;
  if (n > 0) {
    auto cnt = torch::empty({1}, hdr.options().dtype(torch::kInt64));
    if (wh::vidx_renumber_fused(ptr<float>(hdr), n, lookback(hdr.device()), ptr<int64_t>(cnt),
                                cur_stream(hdr)))
      return cnt;
  }
  auto flag = torch::empty({std::max<int64_t>(n, 1)}, hdr.options().dtype(torch::kInt32));
  auto pos = torch::zeros({n + 1}, hdr.options().dtype(torch::kInt64));
  auto stmp = torch::empty({wh::scan_tmp_elems(n)}, pos.options());
  wh::vidx_renumber(ptr<float>(hdr), n, ptr<int32_t>(flag), ptr<int64_t>(pos), ptr<int64_t>(stmp),
                    cur_stream(hdr));
  return pos.narrow(0, n, 1);
}

// WH_TIMING=step: host time per section of a native step, summed and
// printed (mean us per call) every 1000 calls and at exit -- the launch-
// bound small-minibatch path. WH_TIMING=step2: also the absolute
// steady-clock ns of every mark of calls 200..219 (to line up with a
// rocprofv3 kernel trace)
// every live split, so that a process leaving through os._exit (the bin/
// launchers) can still print them: timing_flush()
std::mutex& split_mu() {
  static std::mutex m;
  return m;
}
std::vector<HostSplit*>& live_splits() {
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
// print every live split now (a short run's summary: the splits print every
// 1000 calls and at their step's destruction, which os._exit skips)
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

// -------------------------------------------------------------- metrics
void auc_after_side(c10::DeviceIndex d, hipStream_t s);
static void auc_check(const Tensor& py, const Tensor& label, const Tensor& auc_sum) {
  CHECK_IN(py, torch::kFloat32);
  CHECK_IN(label, torch::kFloat32);
  CHECK_IN(auc_sum, torch::kFloat64);
  TORCH_CHECK(py.numel() == label.numel(), "auc: py/label size mismatch");
  TORCH_CHECK(py.numel() < (int64_t)1 << 30, "auc: at most 2^30 examples per call");
}
// the AUC chain on stream s, which is the current stream (the scratch is its)
static void auc_run(const Tensor& py, const Tensor& label, const Tensor& auc_sum, hipStream_t s) {
  const int64_t n = py.numel();
  const int64_t wsb = wh::auc_ws_bytes(n);
  Tensor scratch;
  if (wsb) scratch = torch::empty({wsb}, py.options().dtype(torch::kUInt8));
  wh::auc_accumulate(ptr<float>(py), ptr<float>(label), n, dev_ws(py.device()).auc.data_ptr(),
                     wsb ? scratch.data_ptr() : nullptr, ptr<double>(auc_sum), s);
}
// auc_sum[0] += exact AUC of (py, label) (sort-free bucketed rank sum)
void auc_acc(const Tensor& py, const Tensor& label, const Tensor& auc_sum) {
  auc_check(py, label, auc_sum);
  c10::DeviceGuard g(py.device());
  auc_after_side(py.device().index(), cur_stream(py));  // (the workspace is shared)
  auc_run(py, label, auc_sum, cur_stream(py));
}

// The same on a per-device side stream owned here (it waits for the current
// stream first; auc_join makes the current stream wait for it): the Python
// form of this (stream objects, wait_stream, a stream context) cost ~30 us
// of host time per minibatch, which bounds small-minibatch training.
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
// submission order (a deterministic sum). Off by default: on the headline
// step (100k rows) it measured level with the device chain (140.0 / 141.9 M
// vs 140.7 / 139.5 M, profiles/round6_p1_isolated.txt), although dropping
// the AUC altogether gains 3-5 % -- the side stream's event pair, the two
// copies and the join remain.
class HostAuc {
 public:
  // the pool new jobs go to (nullptr: the device chain)
  static HostAuc* get() {
    init();
    return on() ? pool() : nullptr;
  }
  // the pool pending jobs are in (also after enable(0))
  static HostAuc* any() {
    init();
    return pool();
  }
  static void enable(int nt) {
    init();
    if (nt > 0 && !pool()) pool() = new HostAuc(nt);
    on() = nt > 0;
  }

  void submit(const float* py, const float* lab, int64_t n, hipStream_t s, const void* target) {
    Job* j = nullptr;
    {
      std::unique_lock<std::mutex> lk(mu_);
      // back-pressure: the host falls this far behind only if its threads are starved
      space_cv_.wait(lk, [&] { return outstanding_ < kMaxOutstanding; });
      ++outstanding_;
      for (size_t k = 0; k < free_.size(); ++k)
        if (free_[k]->cap >= n) {
          j = free_[k];
          free_.erase(free_.begin() + k);
          break;
        }
    }
    if (!j) {
      j = new Job();
      WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&j->ev, hipEventDisableTiming));
    }
    if (j->cap < n) {
      if (j->buf) WH_HIP_CHECK_HOST(hipHostFree(j->buf));
      j->cap = std::max<int64_t>(n, 1 << 17);
      WH_HIP_CHECK_HOST(hipHostMalloc(reinterpret_cast<void**>(&j->buf), 2 * j->cap * sizeof(float),
                                      hipHostMallocDefault));
    }
    j->n = n;
    j->target = target;
    j->done = false;
    WH_HIP_CHECK_HOST(hipMemcpyAsync(j->buf, py, n * sizeof(float), hipMemcpyDeviceToHost, s));
    WH_HIP_CHECK_HOST(hipMemcpyAsync(j->buf + j->cap, lab, n * sizeof(float), hipMemcpyDeviceToHost, s));
    WH_HIP_CHECK_HOST(hipEventRecord(j->ev, s));
    std::lock_guard<std::mutex> lk(mu_);
    j->seq = next_seq_++;
    pending_.push_back(j);
    queue_.push_back(j);
    work_cv_.notify_one();
  }

  bool has(const void* target) {
    std::lock_guard<std::mutex> lk(mu_);
    if (acc_.count(target)) return true;
    for (Job* j : pending_)
      if (j->target == target) return true;
    return false;
  }

  // wait for target's jobs; their AUCs summed in submission order
  double join(const void* target) {
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] {
      for (Job* j : pending_)
        if (j->target == target) return false;
      return true;
    });
    auto it = acc_.find(target);
    if (it == acc_.end()) return 0;
    const double sum = it->second;
    acc_.erase(it);
    return sum;
  }

 private:
  struct Job {
    hipEvent_t ev = nullptr;
    float* buf = nullptr;  // [cap] scores, then [cap] labels
    int64_t cap = 0, n = 0;
    const void* target = nullptr;
    uint64_t seq = 0;
    double result = 0;
    bool done = false;
  };
  static constexpr int kMaxOutstanding = 64;
  static HostAuc*& pool() {
    static HostAuc* p = nullptr;  // never destroyed: os._exit ends the process
    return p;
  }
  static bool& on() {
    static bool b = false;
    return b;
  }
  static void init() {
    static const bool once = [] {
      const char* e = std::getenv("WH_AUC_HOST_THREADS");
      const int nt = e ? std::atoi(e) : 0;
      if (nt > 0) pool() = new HostAuc(nt);
      on() = nt > 0;
      return true;
    }();
    (void)once;
  }

  explicit HostAuc(int nt) {
    for (int t = 0; t < nt; ++t) std::thread([this] { run(); }).detach();
  }

  void run() {
    std::vector<uint64_t> ws;
    for (;;) {
      Job* j;
      {
        std::unique_lock<std::mutex> lk(mu_);
        work_cv_.wait(lk, [&] { return !queue_.empty(); });
        j = queue_.front();
        queue_.pop_front();
      }
      WH_HIP_CHECK_HOST(hipEventSynchronize(j->ev));
      const double r = wh::auc_exact_host(j->buf, j->buf + j->cap, j->n, ws);
      std::lock_guard<std::mutex> lk(mu_);
      j->result = r;
      j->done = true;
      // fold finished jobs into their target's sum in submission order (a
      // deterministic sum) and recycle them, so jobs never wait for a join
      while (!pending_.empty() && pending_.front()->done) {
        Job* f = pending_.front();
        pending_.pop_front();
        acc_[f->target] += f->result;
        free_.push_back(f);
        --outstanding_;
      }
      done_cv_.notify_all();
      space_cv_.notify_all();
    }
  }

  std::mutex mu_;
  std::condition_variable work_cv_, done_cv_, space_cv_;
  std::deque<Job*> queue_;
  std::deque<Job*> pending_;  // submitted, not yet folded (submission order)
  std::map<const void*, double> acc_;  // folded AUC sums per target
  std::vector<Job*> free_;
  uint64_t next_seq_ = 0;
  int outstanding_ = 0;
};

void auc_acc_side(const Tensor& py, const Tensor& label, const Tensor& auc_sum) {
  auc_check(py, label, auc_sum);
  // a small minibatch's AUC is ONE launch of a few microseconds (the
  // pairwise k_auc_small): it runs in order on the current stream, without
  // the side stream's event pair (~4 us of host time in a launch-bound
  // 1000-row step)
  if (py.numel() <= 4096) return auc_acc(py, label, auc_sum);
  c10::DeviceGuard g(py.device());
  AucSide* a = auc_side(py.device().index(), true);
  WH_HIP_CHECK_HOST(hipEventRecord(a->in, cur_stream(py)));
  WH_HIP_CHECK_HOST(hipStreamWaitEvent(a->s.stream(), a->in, 0));
  c10::hip::HIPCachingAllocator::recordStream(py.storage().data_ptr(), a->s);
  c10::hip::HIPCachingAllocator::recordStream(label.storage().data_ptr(), a->s);
  if (HostAuc* h = HostAuc::get()) {  // (the copies touch no shared workspace: not dirty)
    h->submit(ptr<float>(py), ptr<float>(label), py.numel(), a->s.stream(), auc_sum.data_ptr());
    return;
  }
  a->dirty = true;
  c10::hip::HIPStreamGuard sg(a->s);  // the scratch is the side stream's
  auc_run(py, label, auc_sum, a->s.stream());
}

void auc_join(const Tensor& auc_sum) {
  if (!auc_sum.is_cuda()) return;
  c10::DeviceGuard g(auc_sum.device());
  auc_after_side(auc_sum.device().index(), cur_stream(auc_sum));
  HostAuc* h = HostAuc::any();
  if (h && h->has(auc_sum.data_ptr())) {
    const double s = h->join(auc_sum.data_ptr());
    auc_sum.add_(s);
  }
}

Tensor auc(const Tensor& py, const Tensor& label) {
  auto out = torch::zeros({1}, py.options().dtype(torch::kFloat64));
  auc_acc(py, label, out);
  return out;
}

// reference path: rocPRIM radix sort + rank-sum (kept as a cross-check)
Tensor auc_sorted(const Tensor& py, const Tensor& label) {
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

// keys % m (uint64 semantics), returned as a new tensor
Tensor key_mod(const Tensor& keys, int64_t m) {
  CHECK_IN(keys, torch::kInt64);
  TORCH_CHECK(m > 0, "max_key must be positive");
  c10::DeviceGuard g(keys.device());
  auto out = keys.clone();
  wh::key_mod(reinterpret_cast<uint64_t*>(out.data_ptr()), out.numel(), (uint64_t)m,
              cur_stream(keys));
  return out;
}

// ------------------------------------------------------- payload filter
// x [rows, w] f32 -> uint8 [rows, record_bytes]
Tensor quant_rows(const Tensor& x, int64_t nb, int64_t seed) {
  CHECK_IN(x, torch::kFloat32);
  TORCH_CHECK(nb >= 1 && nb <= 3, "fixed_bytes must be 1, 2 or 3");
  TORCH_CHECK(x.dim() == 2, "quant_rows: x must be [rows, w]");
  c10::DeviceGuard g(x.device());
  const int w = (int)x.size(1);
  auto out = torch::empty({x.size(0), wh::quant_record_bytes(w, (int)nb)},
                          x.options().dtype(torch::kUInt8));
  wh::quant_rows(ptr<float>(x), x.size(0), w, (int)nb, (uint64_t)seed, ptr<uint8_t>(out),
                 cur_stream(x));
  return out;
}

Tensor dequant_rows(const Tensor& q, int64_t w, int64_t nb) {
  CHECK_IN(q, torch::kUInt8);
  TORCH_CHECK(nb >= 1 && nb <= 3, "fixed_bytes must be 1, 2 or 3");
  TORCH_CHECK(q.dim() == 2 && q.size(1) == wh::quant_record_bytes((int)w, (int)nb),
              "dequant_rows: bad record size");
  c10::DeviceGuard g(q.device());
  auto x = torch::empty({q.size(0), w}, q.options().dtype(torch::kFloat32));
  wh::dequant_rows(ptr<uint8_t>(q), q.size(0), (int)w, (int)nb, ptr<float>(x), cur_stream(q));
  return x;
}

// region filter of the multi-shard exchange (quant.hip qregion_*): x the
// float layout (flat view), desc int64 [P, 6] on the device, built and
// bounds-checked on the host (kv/psx.py _QFilter) against x / out sizes.
Tensor ps_qpack(const Tensor& x, const Tensor& desc, int64_t rows, int64_t W, int64_t nb,
                int64_t seed) {
  CHECK_IN(x, torch::kFloat32);
  CHECK_IN(desc, torch::kInt64);
  TORCH_CHECK(nb >= 1 && nb <= 3 && W >= 1 && W <= 1024, "ps_qpack: bad record shape");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 6 && desc.size(0) >= 1, "ps_qpack: desc [P, 6]");
  c10::DeviceGuard g(x.device());
  auto out = torch::empty({rows, wh::quant_record_bytes((int)W, (int)nb)},
                          x.options().dtype(torch::kUInt8));
  wh::qregion_pack(ptr<float>(x), ptr<int64_t>(desc), (int)desc.size(0), rows, (int)W, (int)nb,
                   (uint64_t)seed, ptr<uint8_t>(out), cur_stream(x));
  return out;
}

void ps_qunpack(const Tensor& q, const Tensor& desc, int64_t W, int64_t nb, const Tensor& out) {
  CHECK_IN(q, torch::kUInt8);
  CHECK_IN(desc, torch::kInt64);
  CHECK_IN(out, torch::kFloat32);
  TORCH_CHECK(nb >= 1 && nb <= 3 && q.dim() == 2 &&
                  q.size(1) == wh::quant_record_bytes((int)W, (int)nb),
              "ps_qunpack: bad record size");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 6 && desc.size(0) >= 1, "ps_qunpack: desc [P, 6]");
  c10::DeviceGuard g(q.device());
  wh::qregion_unpack(ptr<uint8_t>(q), ptr<int64_t>(desc), (int)desc.size(0), q.size(0), (int)W,
                     (int)nb, ptr<float>(out), cur_stream(q));
}

Tensor trunc_u8(const Tensor& c) {
  CHECK_IN(c, torch::kInt32);
  c10::DeviceGuard g(c.device());
  auto out = torch::empty({c.numel()}, c.options().dtype(torch::kUInt8));
  wh::trunc_u8(ptr<int32_t>(c), c.numel(), ptr<uint8_t>(out), cur_stream(c));
  return out;
}

// ---------------------------------------------------------------- synth
std::vector<Tensor> synth_criteo(int64_t nrows, int64_t seed, int64_t step, const Tensor& card) {
  CHECK_IN(card, torch::kInt64);
  c10::DeviceGuard g(card.device());
  const int nfield = (int)card.numel();
  auto keys = torch::empty({nrows * nfield}, card.options());
  auto label = torch::empty({nrows}, card.options().dtype(torch::kFloat32));
  auto offset = torch::empty({nrows + 1}, card.options());
  wh::synth_criteo(nrows, (uint64_t)seed, (uint64_t)step, ptr<int64_t>(card), nfield,
                   reinterpret_cast<uint64_t*>(keys.data_ptr()), ptr<float>(label),
                   ptr<int64_t>(offset), cur_stream(card));
  return {keys, label, offset};
}

Tensor gather_rows(const Tensor& in, const Tensor& idx) {
  CHECK_IN(in, torch::kFloat32);
  CHECK_IN(idx, torch::kInt32);
  c10::DeviceGuard g(in.device());
  const int64_t width = in.dim() > 1 ? in.numel() / in.size(0) : 1;
  auto out = torch::empty({idx.numel(), width}, in.options());
  wh::gather_rows(ptr<float>(in), ptr<int32_t>(idx), idx.numel(), (int)width, ptr<float>(out),
                  cur_stream(in));
  return in.dim() > 1 ? out : out.view({idx.numel()});
}

}  // namespace wh_bind

PYBIND11_MODULE(_hip, m) {
  m.doc() = "wormhole_amd gfx950 HIP kernels";
  m.def("scan_excl", &scan_excl);
  bind_localize(m);
  bind_fm(m);  // LinearStep, DifactoStep, fm_*, spmv_t (before KVStore: their signatures)
  bind_psx(m);  // RcclComm, PSX_TX_*, PsxStep, a2a_plan, c10d_a2a_rows
  m.def("vidx_renumber", &vidx_renumber);
  m.def("ps_unpack", &ps_unpack);
  m.def("ps_pack_gw", &ps_pack_gw);
  m.def("ps_records", &ps_records);
  m.def("ps_c0", &ps_c0, py::arg("owner_cnt"), py::arg("vcnt"), py::arg("P"), py::arg("flag"),
        py::arg("loopback") = false);
  m.def("auc", &auc);
  m.def("quant_rows", &quant_rows);
  m.def("key_mod", &key_mod);
  m.def("dequant_rows", &dequant_rows);
  m.def("trunc_u8", &trunc_u8);
  m.def("ps_qpack", &ps_qpack, py::arg("x"), py::arg("desc"), py::arg("rows"), py::arg("W"),
        py::arg("nb"), py::arg("seed"));
  m.def("ps_qunpack", &ps_qunpack, py::arg("q"), py::arg("desc"), py::arg("W"), py::arg("nb"),
        py::arg("out"));
  m.def("auc_acc", &auc_acc);
  m.def("auc_acc_side", &auc_acc_side);
  m.def("auc_join", &auc_join);
  m.def("auc_host_threads", [](int n) { HostAuc::enable(n); },
        "large training minibatches' AUC on n host threads (0: the device chain)");
  m.def("timing_flush", &timing_flush);
  m.def("auc_sorted", &auc_sorted);
  m.def("synth_criteo", &synth_criteo);
  m.def("gather_rows", &gather_rows);
  // the stateless families, each from its own translation unit
  bind_bsp(m);
  bind_gbdt(m);
  bind_kmeans(m);
  bind_ingest(m);
  py::class_<KVStore>(m, "KVStore")
      .def(py::init<int64_t, int64_t, int64_t, int64_t>(), py::arg("cap"), py::arg("vcap"),
           py::arg("dim"), py::arg("device"))
      .def("find", &KVStore::find)
      .def("occupied", &KVStore::occupied)
      .def("linear_pull", &KVStore::linear_pull)
      .def("linear_push", &KVStore::linear_push)
      .def("difacto_push_cnt", &KVStore::difacto_push_cnt)
      .def("difacto_pull", &KVStore::difacto_pull)
      .def("difacto_open_pull",
           py::overload_cast<const Tensor&, bool, const c10::optional<Tensor>&,
                             const std::vector<double>&, int64_t, bool, int64_t, bool>(
               &KVStore::difacto_open_pull),
           py::arg("keys"), py::arg("insert"),
           py::arg("cnt"), py::arg("h"), py::arg("threshold"), py::arg("l1_shrk"), py::arg("seed"),
           py::arg("direct") = false)
      .def("difacto_push", &KVStore::difacto_push)
      .def("ps_open", &KVStore::ps_open, py::arg("keys"), py::arg("use_cnt"), py::arg("segS"),
           py::arg("segHS"), py::arg("rows_cap"), py::arg("insert"), py::arg("chains"), py::arg("h"),
           py::arg("threshold"), py::arg("l1_shrk"), py::arg("seed"),
           py::arg("chain_in") = py::none())
      .def("ps_push", &KVStore::ps_push, py::arg("slot"), py::arg("vpos"), py::arg("chain"),
           py::arg("head"), py::arg("segS"), py::arg("segHS"), py::arg("gbuf"), py::arg("h"),
           py::arg("threshold"), py::arg("l1_shrk"), py::arg("seed"),
           py::arg("prep_chain") = py::none(), py::arg("prep_n") = 0)
      .def("ps_push_linear", &KVStore::ps_push_linear, py::arg("slot"), py::arg("chain"),
           py::arg("head"), py::arg("segS"), py::arg("g"), py::arg("algo"), py::arg("alpha"),
           py::arg("beta"), py::arg("l1"), py::arg("l2"), py::arg("t0"),
           py::arg("prep_chain") = py::none(), py::arg("prep_n") = 0)
      .def("grow", &KVStore::grow)
      .def("grow_v", &KVStore::grow_v)
      .def("summary", &KVStore::summary)
      .def("summary_async", &KVStore::summary_async)
      .def("summary_read", &KVStore::summary_read)
      .def_property_readonly("dim", &KVStore::dim)
      .def_property_readonly("vstride", &KVStore::vstride)
      .def_property_readonly("cap", &KVStore::cap)
      .def_property_readonly("vcap", &KVStore::vcap)
      .def_readonly("ps_opens", &KVStore::opens_)
      .def_readonly("slots", &KVStore::slots_)
      .def_readonly("keys", &KVStore::keys_)
      .def_readonly("w", &KVStore::w_)
      .def_readonly("z", &KVStore::z_)
      .def_readonly("sq", &KVStore::sq_)
      .def_readonly("cnt", &KVStore::cnt_)
      .def_readonly("vrow", &KVStore::vrow_)
      .def_readonly("V", &KVStore::V_)
      .def_readonly("VG", &KVStore::VG_)
      .def_readonly("vnext", &KVStore::vnext_)
      .def_property_readonly("stats", [](const KVStore& k) {
        // counters summed over their shards: [8] int64 (a copy)
        return k.stats_.narrow(1, 0, wh::kStatCount).sum(0);
      })
      .def("reset_stats", [](KVStore& k, int64_t i0, int64_t i1) {
        k.stats_.narrow(1, i0, i1 - i0).zero_();
      })
      .def("add_stat", [](KVStore& k, int64_t i, int64_t v) {
        k.stats_.select(1, i).narrow(0, 0, 1).add_(v);
      });
}
