// ------------------------------------------------------ native P=1 step
// (included by hip_ops.cc after localize_ahead.inl)
// The single-shard linear training step in ONE native call (reference
// AsgdWorker::ProcessMinibatch, learn/linear/async_sgd.h:240-288, on one
// server shard): finish this minibatch's localize (begun by the previous
// call) -> begin the next one on the localize stream -> store guard (summary
// of the previous open; device rehash past the load bound) -> find/insert ->
// pull -> forward + loss + metrics -> AUC on its side stream -> backward ->
// push (SGD / AdaGrad / FTRL). At the reference's minibatch of 10000 rows
// the GPU work is ~80 us of kernels per step while the same sequence driven
// from Python cost ~250 us of host time per step; here the host only pays
// the launches.
class LinearStep {
 public:
  // h: 4 words of coherent host memory the summary kernel writes directly
  // (a 32-byte hipMemcpyAsync to pinned memory cost ~40 us of host time)
  struct Summ {
    int64_t* h = nullptr;
    hipEvent_t ev = nullptr;
    int64_t issued = 0;
    bool pending = false;
  };
  static constexpr int kSumm = 4;
  LinearStep(KVStore* store, int64_t algo, double alpha, double beta, double l1, double l2,
             int64_t loss, double max_load, bool direct)
      : store_(store), algo_(algo), alpha_(alpha), beta_(beta), l1_(l1), l2_(l2), loss_(loss),
        max_load_(max_load), ahead_(store->slots_.device()) {
    TORCH_CHECK(store->vstride() == 0, "LinearStep needs a linear store");
    // the localize-free step unless a bitwise-repeatable one is asked for
    // (its per-slot gradient sums are float atomics)
    direct_ = direct && !deterministic();
    dev_ = store->slots_.device().index();
  }
  ~LinearStep() {
    ahead_.reset();
    for (Summ& m : sum_) {
      if (m.ev) (void)hipEventSynchronize(m.ev);
      if (m.ev) (void)hipEventDestroy(m.ev);
      if (m.h) (void)hipHostFree(m.h);
    }
  }

  // one minibatch; returns the predictions py [rows]. next_*: the next
  // call's minibatch, whose localize begins now (on the localize stream,
  // after `ready` -- a hipEvent_t handle of its producer -- or, with 0, after
  // everything queued on the current stream).
  Tensor step(const Tensor& keys, const Tensor& offset, const c10::optional<Tensor>& val,
              const Tensor& label, bool train, const Tensor& met, const Tensor& auc_sum,
              const c10::optional<Tensor>& nkeys, const c10::optional<Tensor>& noffset,
              const c10::optional<Tensor>& nval, int64_t ready) {
    if (use_direct(keys.numel())) {
      reset();  // (a localize begun for this minibatch by a larger one before)
      return step_direct(keys, offset, val, label, train, met, auc_sum, ready);
    }
    // begin the next minibatch's localize only if it will take this path
    const bool nl = nkeys.has_value() && nkeys->defined() && !use_direct(nkeys->numel());
    Tensor py = step_localize(keys, offset, val, label, train, met, auc_sum,
                              nl ? nkeys : c10::nullopt, nl ? noffset : c10::nullopt,
                              nl ? nval : c10::nullopt, nl ? ready : 0);
    if (!nl && ready)  // the next (direct-path) minibatch is read on S after this step
      WH_HIP_CHECK_HOST(hipStreamWaitEvent(cur_stream(keys), reinterpret_cast<hipEvent_t>(ready), 0));
    return py;
  }

  // The localize-free step (csrc/hip/linear_direct.hip): touch (dedup per
  // row tile in LDS, find-or-insert, slot list) -> forward on the slots ->
  // AUC -> per-slot gradient sums -> push over the slot list. No host read;
  // the next minibatch's producer event is waited for at the END of this
  // step's work on S.
  Tensor step_direct(const Tensor& keys, const Tensor& offset, const c10::optional<Tensor>& val,
                     const Tensor& label, bool train, const Tensor& met, const Tensor& auc_sum,
                     int64_t ready) {
    CHECK_IN(keys, torch::kInt64);
    CHECK_IN(offset, torch::kInt64);
    CHECK_IN(label, torch::kFloat32);
    CHECK_IN(met, torch::kFloat64);
    const int64_t nrows = offset.numel() - 1, nnz = keys.numel();
    TORCH_CHECK(label.numel() == nrows, "label size mismatch");
    const float* vp = nullptr;
    if (val.has_value() && val->defined() && val->numel()) {
      CHECK_IN((*val), torch::kFloat32);
      TORCH_CHECK(val->numel() == nnz, "val size mismatch");
      vp = ptr<float>(*val);
    }
    HostTimer ht(timing_.get());
    c10::DeviceGuard g(keys.device());
    const hipStream_t S = cur_stream(keys);
    auto i32 = keys.options().dtype(torch::kInt32);
    // inputs produced on another stream (a data generator / copy stream)
    // are read on S: their blocks are not reused before S is done with them
    {
      auto cs = c10::hip::getCurrentHIPStream(dev_);
      for (const Tensor* x : {&keys, &offset, &label})
        c10::hip::HIPCachingAllocator::recordStream(x->storage().data_ptr(), cs);
      if (vp) c10::hip::HIPCachingAllocator::recordStream(val->storage().data_ptr(), cs);
    }
    ht.mark(0);
    // store guard: the previous step's summary (long complete), then room
    // for every id of this minibatch to be new
    if (train) guard_before(nnz);
    if (!grad_.defined() || grad_.numel() < store_->cap())
      grad_ = torch::zeros({store_->cap()}, keys.options().dtype(torch::kFloat32));
    // the overflow list's counter: zero between steps (the push re-zeroes it)
    if (!ovf_cnt_.defined()) ovf_cnt_ = torch::zeros({1}, i32);
    ht.mark(1);
    // one int32 block (slot per non-zero | per-tile slot lists | overflow
    // list | per-tile counts) and one float block (py | dual)
    const int R = wh::ld_rows_per_tile(nnz, nrows);
    const int T = wh::ld_tile_table(nnz);
    const int64_t nz1 = std::max<int64_t>(nnz, 1);
    const int64_t ntiles = nrows > 0 ? (nrows + R - 1) / R : 0;
    auto iws = torch::empty({2 * nz1 + ntiles * (T + 1)}, i32);
    int32_t* lid = ptr<int32_t>(iws);
    int32_t* ovf = lid + nz1;
    int32_t* tlist = ovf + nz1;
    unsigned int* tcnt = reinterpret_cast<unsigned int*>(tlist + ntiles * T);
    unsigned int* ovf_cnt = reinterpret_cast<unsigned int*>(ovf_cnt_.data_ptr());
    auto fws = torch::empty({2 * std::max<int64_t>(nrows, 1)}, keys.options().dtype(torch::kFloat32));
    auto py = fws.narrow(0, 0, nrows);
    float* dual = ptr<float>(fws) + std::max<int64_t>(nrows, 1);
    auto part = torch::empty({wh::fm_fwd_partials()}, met.options());
    ht.mark(2);
    ++stamp_;
    if (stamp_ == 0) stamp_ = 1;
    wh::KVTable t = store_->table();
    wh::ld_touch(t, reinterpret_cast<const uint64_t*>(keys.data_ptr()), ptr<int64_t>(offset),
                 nrows, nnz, R, stamp_, train ? 1 : 0, lid, tlist, tcnt, ovf, ovf_cnt, S);
    ht.mark(3);
    if (train) guard_after(S, nnz);
    ht.mark(4);
    const int lossf = (int)loss_ | (met.numel() >= 5 ? 256 : 0);
    wh::lin_forward_strided(nrows, ptr<int64_t>(offset), lid, vp,
                            reinterpret_cast<const float*>(t.sl) + 2, 8, ptr<float>(label), lossf,
                            ptr<float>(fws), dual, ptr<double>(met), ptr<double>(part),
                            ptr<unsigned int>(dev_ws(keys.device()).fwd_ticket), S);
    ht.mark(5);
    if (train && nnz > 0) {
      wh::ld_backward(lid, vp, ptr<int64_t>(offset), nrows, nnz, R, dual, ptr<float>(grad_), S);
      ++pushes_;
      wh::LinearHP hp{(int)algo_, (float)alpha_, (float)beta_, (float)l1_, (float)l2_,
                      (float)((beta_ + std::sqrt((double)pushes_)) / alpha_)};
      wh::ld_push(t, ntiles, T, tlist, tcnt, ovf, ovf_cnt, ptr<float>(grad_), hp, S);
    }
    ht.mark(6);
    // the AUC side stream is enqueued last: its host work (event, stream
    // switch) no longer sits between the forward and backward launches
    auc_acc_side(py, label, auc_sum);
    ht.mark(7);
    // the next minibatch (produced on another stream) is read by S after
    // this step's work: order S after its producer now
    if (ready) WH_HIP_CHECK_HOST(hipStreamWaitEvent(S, reinterpret_cast<hipEvent_t>(ready), 0));
    ht.mark(8);
    return py;
  }

  Tensor step_localize(const Tensor& keys, const Tensor& offset, const c10::optional<Tensor>& val,
                       const Tensor& label, bool train, const Tensor& met, const Tensor& auc_sum,
                       const c10::optional<Tensor>& nkeys, const c10::optional<Tensor>& noffset,
                       const c10::optional<Tensor>& nval, int64_t ready) {
    c10::DeviceGuard g(keys.device());
    const hipStream_t S = cur_stream(keys);
    // this minibatch's localize
    std::vector<Tensor> loc = ahead_.take(keys, offset, val, S);
    const Tensor &uniq = loc[0], &lid = loc[3], &csc_off = loc[4], &csc_row = loc[5],
                 &csc_val = loc[6];
    const int64_t U = uniq.numel();
    // the next minibatch's localize, on its own stream behind everything
    // queued on S so far (its outputs may reuse blocks S still reads)
    if (nkeys.has_value() && nkeys->defined()) ahead_.begin(*nkeys, *noffset, nval, ready, S);
    // store guard: the previous open's summary (long complete), then room
    // for this open's inserts
    if (train) guard_before(U);
    Tensor slot = store_->find(uniq, train);
    if (train) guard_after(S, U);
    Tensor w = store_->linear_pull(slot);
    auto fw = fm_forward(offset, lid, val, w, c10::nullopt, 0, label, loss_, met);
    auc_acc_side(fw[0], label, auc_sum);
    if (train && U > 0) {
      auto bw = fm_backward(csc_off, csc_row,
                            csc_val.numel() ? c10::optional<Tensor>(csc_val) : c10::nullopt,
                            fw[1], c10::nullopt, w, c10::nullopt, 0);
      ++pushes_;
      const double eta = (beta_ + std::sqrt((double)pushes_)) / alpha_;
      store_->linear_push(slot, bw[0], algo_, alpha_, beta_, l1_, l2_, eta);
    }
    return fw[0];
  }

  // drop a begun localize (end of a pass)
  void reset() { ahead_.reset(); }

  // ---- store guard without a per-step host wait: table summaries (keys,
  // failed inserts) are read when their event has completed (polled), the
  // key count in between is bounded by the inserts issued since; only a
  // table close to its load bound waits for the newest summary before
  // deciding to grow (nothing in flight references old slots: a grow is
  // stream-ordered before this step's inserts)
  void guard_read(Summ& m) {
    const volatile int64_t* h = m.h;
    m.pending = false;
    TORCH_CHECK(h[1] == 0, "parameter store shard lost data: ", h[1], " failed inserts (table ",
                h[0], "/", store_->cap(), " keys)");
    if (m.issued >= base_issued_) {
      base_keys_ = h[0];
      base_issued_ = m.issued;
    }
  }
  void guard_poll(bool block) {
    for (Summ& m : sum_) {
      if (!m.pending) continue;
      if (block) WH_HIP_CHECK_HOST(hipEventSynchronize(m.ev));
      else if (hipEventQuery(m.ev) != hipSuccess) continue;
      guard_read(m);
    }
  }
  int64_t keys_bound() const { return base_keys_ + (issued_ - base_issued_); }
  void guard_before(int64_t n_new) {
    guard_poll(false);
    if (wh::grown_cap(keys_bound() + n_new, store_->cap(), max_load_) == store_->cap()) return;
    guard_poll(true);  // the exact count before growing
    const int64_t cap = wh::grown_cap(keys_bound() + n_new, store_->cap(), max_load_);
    if (cap != store_->cap()) {
      store_->grow(cap);
      ++grows_;
    }
  }
  // A summary (a kernel and a 32-byte read-back on the compute stream) every
  // kGuardEvery steps, or every step once the bound nears the load limit:
  // between summaries the bound grows by the inserts issued, so a late
  // summary only makes the grow decision more conservative, and a failed
  // insert still stops training within kGuardEvery steps (and at the flush).
  static constexpr int kGuardEvery = 8;
  void guard_after(hipStream_t S, int64_t n_new, bool force = false) {
    issued_ += n_new;
    const double lim = max_load_ * (double)store_->cap();
    if (!force && ++guard_step_ % kGuardEvery != 0 &&
        keys_bound() + (double)n_new * kGuardEvery < 0.9 * lim)
      return;
    Summ& m = sum_[sum_i_];
    sum_i_ = (sum_i_ + 1) % kSumm;
    if (m.pending) {  // (the GPU is kSumm steps behind: wait for the oldest)
      WH_HIP_CHECK_HOST(hipEventSynchronize(m.ev));
      guard_read(m);
    }
    if (!m.h) {
      void* p = nullptr;
      WH_HIP_CHECK_HOST(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent));
      m.h = static_cast<int64_t*>(p);
      std::memset(p, 0, 64);
      WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&m.ev, hipEventDisableTiming));
    }
    wh::kv_summary(store_->table(), m.h, S);
    WH_HIP_CHECK_HOST(hipEventRecord(m.ev, S));
    m.issued = issued_;
    m.pending = true;
  }

  // a summary now, waited for: raises on a failed insert (end of a pass,
  // before the model is read)
  void guard_sync() {
    c10::DeviceGuard g(store_->slots_.device());
    guard_after(c10::hip::getCurrentHIPStream(dev_).stream(), 0, true);
    guard_poll(true);
  }

  int64_t grows() const { return grows_; }
  bool direct() const { return direct_; }
  // the localize-free step pays off while a minibatch is small (launch- and
  // latency-bound: the reference's 10000 rows: 71.0 vs 55.1 M ex/s); above
  // 600k non-zeros (~15k Criteo rows; at 25k rows the localize path is
  // ahead, 129 vs 109 M ex/s) the localize's global dedup does fewer table
  // probes and atomics than per-tile dedup
  bool use_direct(int64_t nnz) const { return direct_ && nnz <= 600000; }
  int64_t pushes() const { return pushes_; }
  void set_pushes(int64_t p) { pushes_ = p; }

 private:
  KVStore* store_;
  int64_t algo_;
  double alpha_, beta_, l1_, l2_;
  int64_t loss_;
  double max_load_;
  int dev_ = 0;
  LocalizeAhead ahead_;
  bool direct_ = true;
  // direct step: per-slot gradient sums (all zero between steps), the
  // overflow slot list's counter (zero between steps)
  Tensor grad_, ovf_cnt_;
  uint32_t stamp_ = 0;
  std::unique_ptr<HostSplit> timing_{host_split("linear direct step")};
  int64_t guard_step_ = 0;
  Summ sum_[kSumm];
  int sum_i_ = 0;
  int64_t issued_ = 0, base_keys_ = 0, base_issued_ = 0;
  int64_t grows_ = 0, pushes_ = 0;
};
