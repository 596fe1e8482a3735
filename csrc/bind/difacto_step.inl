// The single-shard DiFacto training / evaluation step in ONE native call
// (included by hip_ops.cc after linear_step.inl; the Python twin, kept
// as the CPU path and the test oracle, is models/difacto.py
// DifactoLearner.process with WH_DIFACTO_NATIVE=0).
//
// Reference per-minibatch flow: learn/difacto/async_sgd.h:363-425 on one
// server shard -- push the feature counts (data pass 0) -> pull w and the
// lazily allocated V rows -> FM forward + loss + AUC -> FM backward ->
// gradient clipping / dropout / normalization (learn/difacto/loss.h:145-155)
// -> push (FTRL on w, AdaGrad on V). The Python step spent ~150 us of host
// time per call at the reference tutorial's minibatch of 1000 rows
// (learn/difacto/guide/criteo.conf, doc/tutorial/criteo_kaggle.rst:115-131):
// a dozen op calls, each with its argument parsing, stream bookkeeping and
// allocations, for a GPU step of a few tens of microseconds. Here the same
// kernels are enqueued from C++ with one Python crossing per minibatch.
//
// Launch sequence of a training minibatch on S: open / pull -> forward ->
// (V-chunk bucketing) -> backward (scalar chunks, V chunks) -> push; the AUC
// chain starts behind the backward on its side stream.
//
// The backward's chunk plan comes from the open: the backward's outputs and
// scratch are allocated first (fm_bwd_alloc; after the guard, which may grow
// the slab that gvc mirrors in direct mode), the open -- which decides each
// key's embedding row, has the planner's 1024-key tiles and runs a look-back
// scan already -- counts and emits the chunks with the planner's own emit_key
// (wh_chunk_plan.h), and fm_backward runs with FmBwdPhase::kBucketRun. The
// open's fallbacks (more keys than the look-back has tiles, where it also
// takes the compact pull; evaluation passes have no backward) leave planning
// to fm_backward (kAll), as before.
//
// Fused V update (fused_v, the default in direct mode): most embedded keys
// occur at most kChunkV = 64 times in a minibatch, so one backward wave holds
// the key's finished gradient row and its V row in registers. That wave applies
// the AdaGrad step in place (fm.hip k_bwd_v<G, true>) instead of writing the
// row to gvc for the push to read back beside a second read of V; the push
// then skips those keys' row work (FTRL on w and fresh rows are unchanged).
// Direct mode has no clipping / dropout / normalisation, the only readers of
// the compact gradient rows between the backward and the push.
//
// Streams: the compute stream S (the caller's) and the localize stream ls,
// where the NEXT minibatch's localize runs while this one trains
// (LocalizeAhead, as in LinearStep::step_localize); the AUC runs on the
// native AUC side stream.
class DifactoStep {
 public:
  // hp: the learner's 8 DiFacto hyper-parameters; post = (grad_clipping,
  // dropout, grad_normalization, dim); direct: the FM kernels read the V
  // rows in place in the store's slab (no post-processing); fused_v: in
  // direct mode, single-chunk keys get their V update in the backward
  DifactoStep(KVStore* store, std::vector<double> hp, int64_t threshold, bool l1_shrk,
              int64_t seed, int64_t loss, std::vector<double> post, double max_load, bool direct,
              bool fused_v)
      : store_(store), hp_(std::move(hp)), threshold_(threshold), l1_shrk_(l1_shrk), seed_(seed),
        loss_(loss), guard_(store, max_load), ahead_(store->slots_.device()) {
    TORCH_CHECK(hp_.size() == 8 && post.size() == 4, "DifactoStep: hp[8], post[4]");
    vs_ = store->vstride();
    TORCH_CHECK(vs_ > 0, "DifactoStep: an embedding store (vstride > 0)");
    clip_ = post[0];
    dropout_ = post[1];
    gnorm_ = post[2] != 0.0;
    dim_ = (int64_t)post[3];
    post_on_ = clip_ > 0 || dropout_ > 0 || gnorm_;
    direct_ = direct && !post_on_;
    fused_v_ = fused_v && direct_;
  }
  DifactoStep(const DifactoStep&) = delete;
  DifactoStep& operator=(const DifactoStep&) = delete;
  ~DifactoStep() {
    if (timing_) timing_->print();
    ahead_.reset();
    (void)hipDeviceSynchronize();  // (the members' events are destroyed after this)
  }

  // One minibatch. train: insert / count / push (else an evaluation pass:
  // find only, AUC on S). step: the learner's step counter (the dropout
  // seed). next_*: the next call's minibatch, whose localize begins now on
  // the localize stream (after `ready`, a hipEvent_t of its producer, or
  // with 0 after everything queued on S). Returns (py, unique keys,
  // embedding rows as a device int64 [1]).
  py::tuple step(const Tensor& keys, const Tensor& offset, const c10::optional<Tensor>& val,
                 const Tensor& label, bool train, int64_t data_pass, const Tensor& met,
                 const Tensor& auc_sum, int64_t step, const c10::optional<Tensor>& nkeys,
                 const c10::optional<Tensor>& noffset, const c10::optional<Tensor>& nval,
                 int64_t ready) {
    c10::DeviceGuard g(keys.device());
    // WH_TIMING=step: s0 localize finish, s1 next localize begin, s2 guard +
    // open/pull, s3 forward, s4 backward + post, s5 push, s6 AUC
    HostTimer ht(timing_.get());
    const hipStream_t S = cur_stream(keys);
    std::vector<Tensor> loc = ahead_.take(keys, offset, val, S);
    const Tensor &uniq = loc[0], &ucnt = loc[1], &lid = loc[3], &csc_off = loc[4],
                 &csc_row = loc[5], &csc_val = loc[6];
    const int64_t U = uniq.numel();
    ht.mark(0);
    // open + pull (DifactoLearner.process: kv.difacto_open_pull), the
    // feature counts pushed on data pass 0
    const bool push_cnt = train && data_pass == 0;
    if (train) guard_.before(U);  // (no slot is held across steps: nothing to remap)
    // training: the backward's outputs and scratch exist before the open,
    // which writes the chunk plan into them (after the guard: gvc mirrors
    // the V slab in direct mode)
    std::vector<Tensor> bwd;
    wh::FmBwdPlanDst dst;
    bool planned = false;
    if (train && U > 0) {
      bwd = fm_bwd_alloc(csc_off, csc_row.numel(), direct_ ? store_->V_.size(0) : U, vs_, true);
      dst = fm_bwd_plan_dst(bwd, csc_off, csc_row.numel(), label.numel(), vs_);
    }
    auto o = store_->difacto_open_pull(uniq, train,
                                       push_cnt ? c10::optional<Tensor>(ucnt) : c10::nullopt, hp_,
                                       threshold_, l1_shrk_, seed_, direct_,
                                       train && U > 0 ? &dst : nullptr, &planned);
    if (train) guard_.after();  // on S: one wave that reads counters only
    const Tensor &slot = o[0], &hdr = o[1], &vc = o[2], &vpos = o[3];
    ht.mark(2);
    // the next minibatch's localize, right after the pull's launch
    if (nkeys.has_value() && nkeys->defined()) ahead_.begin(*nkeys, *noffset, nval, ready, S);
    ht.mark(1);
    const c10::optional<Tensor> v =
        val.has_value() && val->defined() && val->numel() ? val : c10::nullopt;
    auto fw = fm_forward(offset, lid, v, hdr, vc, vs_, label, loss_, met);
    if (!train) auc_acc(fw[0], label, auc_sum);
    ht.mark(3);
    Tensor m = vpos.narrow(0, vpos.numel() - 1, 1);
    if (train && U > 0) {
      const c10::optional<Tensor> cv =
          csc_val.defined() && csc_val.numel() ? c10::optional<Tensor>(csc_val) : c10::nullopt;
      // (the slabs' addresses are this step's: the guard grows them before the open)
      const FmFuse fuse = {ptr<float>(store_->V_), ptr<float>(store_->VG_),
                           KVStore::dhp(hp_, threshold_, l1_shrk_, seed_)};
      // (the open's compact-pull fallback hands out a copy of the rows: unfused)
      const bool fuse_now = fused_v_ && vc.data_ptr() == store_->V_.data_ptr();
      auto bw = fm_backward_impl(csc_off, csc_row, cv, fw[1], fw[2], hdr, vc, vs_,
                                 fuse_now ? &fuse : nullptr, planned ? &bwd : nullptr);
      if (post_on_)
        fm_grad_post(bw[1], m, dim_, clip_, dropout_, seed_ + 7919 * step + 1, gnorm_);
      ht.mark(4);
      // (the AUC side stream starts behind the backward: its kernels overlap
      // the push and the next open rather than the backward planning)
      auc_acc_side(fw[0], label, auc_sum);
      ht.mark(6);
      store_->difacto_push_after(slot, hdr, bw[0], bw[1], hp_, threshold_, l1_shrk_, seed_,
                                 fuse_now ? c10::optional<Tensor>(ucnt) : c10::nullopt);
      ht.mark(5);
    } else if (train) {
      auc_acc_side(fw[0], label, auc_sum);
    }
    return py::make_tuple(fw[0], U, m);
  }

  // drop a begun localize (end of a pass, or before a Python-path call)
  void reset() { ahead_.reset(); }
  bool direct() const { return direct_; }
  bool fused_v() const { return fused_v_; }
  int64_t grows() const { return guard_.grows(); }
  int64_t vgrows() const { return guard_.vgrows(); }
  // the guard's last summary {keys, failed inserts, V overflows, V rows}
  std::vector<int64_t> guard_sync() {
    if (guard_.stale()) guard_.after();
    return guard_.sync();
  }

 private:
  KVStore* store_;
  std::vector<double> hp_;
  int64_t threshold_;
  bool l1_shrk_;
  int64_t seed_, loss_;
  int vs_ = 0;
  double clip_ = 0, dropout_ = 0;
  bool gnorm_ = false, post_on_ = false, direct_ = false, fused_v_ = false;
  int64_t dim_ = 0;
  StoreGuard guard_;
  LocalizeAhead ahead_;
  std::unique_ptr<HostSplit> timing_{host_split("difacto native step")};
};
