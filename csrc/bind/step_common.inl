// Host logic the native steps share (included by hip_ops.cc before
// linear_step.inl, psx_native.inl and difacto_step.inl): the store guard of
// DifactoStep and PsxStep, and the localize look-ahead of LinearStep and
// DifactoStep.

// ---- store guard (kv/__init__.py StoreGuard is the Python twin and the
// oracle; the arithmetic is host/store_guard_plan.h): before an open the
// previous summary (one open behind, long complete) is checked -- a lost key
// or row raises -- and the table / V slab grow so the coming open, and the
// pushes still in flight, cannot overflow them; after the open the next
// summary is enqueued. Summary slots 2 / 3 of the store (0 / 1 belong to the
// Python guard).
class StoreGuard {
 public:
  StoreGuard(KVStore* store, double max_load)
      : store_(store), max_load_(max_load), dev_(store->slots_.device().index()) {
    c10::DeviceGuard g(store->slots_.device());
    for (auto& e : ev_) WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  StoreGuard(const StoreGuard&) = delete;
  StoreGuard& operator=(const StoreGuard&) = delete;
  ~StoreGuard() {
    for (auto& e : ev_) (void)hipEventDestroy(e);
  }

  // Room for an open of n keys. Returns the old -> new slot map when the
  // table grew (for slot ids held across steps), else an undefined tensor.
  Tensor before(int64_t n) {
    read();
    Tensor remap;
    const int64_t cap = wh::grown_cap(plan_.need(n), store_->cap(), max_load_);
    if (cap != store_->cap()) {
      remap = store_->grow(cap);
      ++grows_;
    }
    if (store_->vstride() > 0 && plan_.vneed(n) > store_->vcap()) {
      store_->grow_v(wh::grown_vcap(plan_.vneed(n), store_->vcap()));
      ++vgrows_;
    }
    plan_.opened(n);
    return remap;
  }
  // The next summary, on the current stream (one wave that reads counters
  // only). No open lies between this and the read that applies it, which
  // zeroes the plan's `since`.
  void after() {
    k_ ^= 1;
    store_->summary_async(2 + k_);
    WH_HIP_CHECK_HOST(hipEventRecord(ev_[k_], c10::hip::getCurrentHIPStream(dev_).stream()));
    pend_ = true;
    issued_ = true;
  }
  // a summary is awaited: the next before() / sync() may wait on the host
  bool pending() const { return pend_; }
  // summaries were taken and the last one has been read (nothing newer known)
  bool stale() const { return issued_ && !pend_; }
  // the last summary {keys, failed inserts, V overflows, V rows}, read now if
  // one is pending
  std::vector<int64_t> sync() {
    read();
    return {plan_.keys, 0, 0, plan_.vused};
  }
  int64_t grows() const { return grows_; }
  int64_t vgrows() const { return vgrows_; }

 private:
  void read() {
    if (!pend_) return;
    wait_event(ev_[k_]);
    pend_ = false;
    auto h = store_->summary_read(2 + k_);
    plan_.summarised(h[0], h[3]);
    TORCH_CHECK(h[1] == 0 && h[2] == 0, "parameter store shard lost data: ", h[1],
                " failed inserts, ", h[2], " embedding rows dropped (table ", h[0], "/",
                store_->cap(), " keys, V slab ", h[3], "/", store_->vcap(), " rows)");
  }

  KVStore* store_;
  double max_load_;
  c10::DeviceIndex dev_;
  wh::StoreGuardPlan plan_;
  hipEvent_t ev_[2] = {};
  int k_ = 0;
  bool pend_ = false, issued_ = false;
  int64_t grows_ = 0, vgrows_ = 0;
};

// ---- localize look-ahead: the NEXT minibatch's localize begins on the
// localize stream while this one trains on the compute stream S; the next
// call takes its outputs, or localizes on S when no job was begun for its
// minibatch. Both streams use the device's localize workspace
// (localize_ops.cc; the job's interface is localize_job.h).
class LocalizeAhead {
 public:
  explicit LocalizeAhead(const c10::Device& device) : dev_(device.index()) {
    c10::DeviceGuard g(device);
    ls_ = c10::hip::getStreamFromExternal(own_stream(dev_, kStreamLinearLs), dev_);
    WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&ev_s_, hipEventDisableTiming));
    WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&ev_ls_, hipEventDisableTiming));
  }
  LocalizeAhead(const LocalizeAhead&) = delete;
  LocalizeAhead& operator=(const LocalizeAhead&) = delete;
  ~LocalizeAhead() {
    job_.reset();
    (void)hipEventDestroy(ev_s_);
    (void)hipEventDestroy(ev_ls_);
  }

  // this minibatch's localize (LocalizeJob::finish's outputs), on S
  std::vector<Tensor> take(const Tensor& keys, const Tensor& offset,
                           const c10::optional<Tensor>& val, hipStream_t S) {
    std::vector<Tensor> loc;
    if (job_ && job_keys_.is_same(keys)) {
      loc = job_->finish();
      // a hash-path job emptied its scratch table on S: the next job on the
      // localize stream (which may reuse that table) waits for S
      if (!job_->partitioned()) s_job_ = true;
      // the job's outputs were allocated on the localize stream and are read
      // on S from here on: their blocks go back to the localize stream's
      // pool only once S's queued work is done (so the localize stream
      // never has to wait for S before the next job)
      for (const Tensor& t : loc)
        if (t.defined() && t.is_cuda() && t.numel()) record(t, false);
    } else {
      // (no job begun for this minibatch) localize on S, after any job still
      // running on the localize stream
      if (job_) {
        WH_HIP_CHECK_HOST(hipEventRecord(ev_ls_, ls_.stream()));
        WH_HIP_CHECK_HOST(hipStreamWaitEvent(S, ev_ls_, 0));
      }
      job_.reset();
      LocalizeJob j(keys, offset, val, 1, hint_, py::none());
      loc = j.finish();
      s_job_ = true;
    }
    reset();
    hint_ = loc[0].numel();
    return loc;
  }

  // Begin the next minibatch's localize on the localize stream, behind
  // `ready` (a hipEvent_t handle of the minibatch's producer) or, with 0,
  // behind everything queued on S so far.
  void begin(const Tensor& nk, const Tensor& no, const c10::optional<Tensor>& nval, int64_t ready,
             hipStream_t S) {
    // the localize stream waits for S when a localize ran on S (the
    // workspace is S's until then) or when the next minibatch has no
    // producer event: it was then made on S (slices, offset rebasing, the
    // handover from a parse stream), possibly by work queued just now
    if (s_job_ || !ready) {
      WH_HIP_CHECK_HOST(hipEventRecord(ev_s_, S));
      WH_HIP_CHECK_HOST(hipStreamWaitEvent(ls_.stream(), ev_s_, 0));
      s_job_ = false;
    }
    if (ready) WH_HIP_CHECK_HOST(hipStreamWaitEvent(ls_.stream(), reinterpret_cast<hipEvent_t>(ready), 0));
    // read on the localize stream now and on the current one by the next step
    record(nk, true);
    record(no, true);
    c10::optional<Tensor> nv;
    if (nval.has_value() && nval->defined() && nval->numel()) {
      nv = *nval;
      record(*nval, true);
    }
    c10::hip::HIPStreamGuard sg(ls_);
    job_ = std::make_unique<LocalizeJob>(nk, no, nv, 1, hint_, py::none());
    job_keys_ = nk;
  }

  // drop a begun localize (end of a pass, or before a step on another path)
  void reset() {
    job_.reset();
    job_keys_ = Tensor();
  }

 private:
  // t's block is not reused before the current stream (and the localize
  // stream) are done with the work queued so far
  void record(const Tensor& t, bool on_ls) {
    if (on_ls) c10::hip::HIPCachingAllocator::recordStream(t.storage().data_ptr(), ls_);
    c10::hip::HIPCachingAllocator::recordStream(t.storage().data_ptr(),
                                                c10::hip::getCurrentHIPStream(dev_));
  }

  c10::DeviceIndex dev_;
  c10::hip::HIPStream ls_ = c10::hip::getDefaultHIPStream();
  hipEvent_t ev_s_ = nullptr, ev_ls_ = nullptr;
  std::unique_ptr<LocalizeJob> job_;
  Tensor job_keys_;
  bool s_job_ = false;  // a localize used the workspace on S since the last begin
  int64_t hint_ = 0;    // the last minibatch's unique keys (the job's table size)
};
