// The localize job: a minibatch's global keys -> (unique keys, local ids,
// CSC) on the device, with one host read. Defined in localize_ops.cc; used by
// the native steps (LocalizeAhead, localize_ahead.h, of the single-shard
// steps in fm_ops.cc; PsxStep in psx_ops.cc) and bound to Python as
// _hip.LocalizeJob / _hip.localize.
#pragma once
#include "bind_common.h"

#include <functional>
#include <tuple>

namespace wh_bind {

// The count exchange of a localize job issued from C++ (kv/psx.py's C0,
// ported by PsxStep): returns (payload [owner_cnt (nshard+1) | stride values
// per peer | extra], the stream the payload is ready on, stride, world).
using NativeExchange =
    std::function<std::tuple<Tensor, hipStream_t, int64_t, int64_t>(const Tensor&)>;

struct LocPinnedRead;  // localize_ops.cc: a pinned count buffer + its event

// finish() returns (uniq i64[U], ucnt i32[U], owner_cnt i64[P], lid i32[nnz],
//                   csc_off i64[U+1], csc_row i32[nnz], csc_val f32[nnz|0],
//                   recv i64[2W|0])
//
// exchange (multi-rank): a callable that takes the device owner counts
// i64[nshard + 1] (last = table-overflow count) and returns the device i64
// [2W] {count from rank q, overflow flag of rank q} of a count all-to-all
// (or kv/psx.py's extended 4-tuple: see from_python; from C++, a
// NativeExchange). It runs before the one host read, so the read returns
// both this rank's counts and its peers' (one synchronisation per minibatch
// instead of two). Every rank sees every rank's overflow flag, so all ranks
// retry together.
//
// Two phases, so that a caller can hide the host read: the constructor
// enqueues the hash insert (or the whole partitioned localize), the owner
// counts, the count exchange and an ASYNC copy of the counts into pinned host
// memory (+ an event); finish() waits for that event only, sizes the outputs
// and enqueues the rest. A learner begins minibatch i+1 right after finishing
// minibatch i, so the wait overlaps i's training.
class LocalizeJob {
 public:
  // defer_exchange: enqueue the localize kernels now, but call the count
  // exchange (and its async host read) only at exchange(): the multi-shard
  // step begins the next minibatch's localize early on its own stream and
  // issues its count collective later, once the payload it carries (the V
  // row counts of this minibatch's open) exists.
  // form: names the exchange's kind in the payload check's message.
  LocalizeJob(const Tensor& keys, const Tensor& offset, const c10::optional<Tensor>& val,
              int64_t nshard, int64_t hint, NativeExchange nex, bool defer_exchange,
              const char* form = "native");
  // exchange: None or a Python callable (see from_python)
  LocalizeJob(const Tensor& keys, const Tensor& offset, const c10::optional<Tensor>& val,
              int64_t nshard, int64_t hint, py::object exchange, bool defer_exchange = false)
      : LocalizeJob(keys, offset, val, nshard, hint, from_python(std::move(exchange)),
                    defer_exchange, "extended") {}
  LocalizeJob(const LocalizeJob&) = delete;
  LocalizeJob& operator=(const LocalizeJob&) = delete;
  ~LocalizeJob();

  // the deferred count exchange (a no-op unless defer_exchange was given)
  void exchange();

  // The one host read: waits for the count exchange (retrying the whole
  // begin at the safe table size if any rank overflowed) and returns the
  // host (owner counts [nshard], everything the exchange appended). A
  // caller may enqueue unrelated work between counts() and finish().
  std::vector<Tensor> counts();

  // the partitioned path: every output is produced on the job's stream
  // before the count read. (The hash path finishes on the caller's stream
  // and returns its scratch table to the device pool from there: a job
  // begun later on another stream must be ordered after that finish.)
  bool partitioned() const { return part_; }

  std::vector<Tensor> finish();

 private:
  static NativeExchange from_python(py::object exchange);
  // what a job may hold in the device's localize workspace
  enum : unsigned { kRead = 1, kInflight = 2, kTable = 4, kAll = 7 };
  void release(unsigned what);
  void enqueue();
  Tensor enqueue_part();
  Tensor enqueue_hash();
  void exchange_and_read();

  Tensor keys_, offset_, val_;
  int64_t nshard_, nnz_ = 0, safe_ = 0, tsize_ = 0, nrecv_ = 0, stride_ = 2;
  NativeExchange nex_;  // empty: a single rank, no exchange
  const char* form_;
  bool defer_ = false, exchanged_ = false;
  Tensor owner_cnt_;
  int tab_ = -1;  // the hash path's slot of the device's table pool
  bool done_ = false;
  Tensor tkeys_, slot_of_, blkoff_, dev_counts_, owner_cnt_h_, recv_h_;
  Tensor uniq_, ucnt_, csc_off_, csc_row_, csc_val_, lid_;  // partitioned path outputs
  wh::PartPlan plan_{};
  bool part_ = false;
  bool counted_ = false;         // in the workspace's in-flight count
  LocPinnedRead* rd_ = nullptr;  // the count read's pinned buffer + event
};

}  // namespace wh_bind
