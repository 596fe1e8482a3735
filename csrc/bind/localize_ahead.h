// The localize look-ahead of the single-shard steps (LinearStep and
// DifactoStep, fm_ops.cc): the NEXT minibatch's localize begins on the
// localize stream while this one trains on the compute stream S; the next
// call takes its outputs, or localizes on S when no job was begun for its
// minibatch. Both streams use the device's localize workspace
// (localize_ops.cc; the job's interface is localize_job.h).
#pragma once
#include "localize_job.h"
#include "step_rt.h"

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>

#include <memory>

namespace wh_bind {

class LocalizeAhead {
 public:
  explicit LocalizeAhead(const c10::Device& device) : dev_(device.index()) {
    c10::DeviceGuard g(device);
    ls_ = c10::hip::getStreamFromExternal(own_stream(dev_, kStreamLinearLs), dev_);
    ev_s_.create();
    ev_ls_.create();
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
    const c10::optional<Tensor> nv = present(nval) ? nval : c10::nullopt;
    if (nv) record(*nv, true);
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
  Event ev_s_, ev_ls_;  // (declared before job_: the job goes first)
  std::unique_ptr<LocalizeJob> job_;
  Tensor job_keys_;
  bool s_job_ = false;  // a localize used the workspace on S since the last begin
  int64_t hint_ = 0;    // the last minibatch's unique keys (the job's table size)
};

}  // namespace wh_bind
