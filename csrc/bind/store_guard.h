// The store guard of the native steps DifactoStep (fm_ops.cc) and PsxStep
// (psx_ops.cc).
#pragma once
#include "kv_store.h"

#include "host/store_guard_plan.h"

namespace wh_bind {

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
    for (auto& e : ev_) e.create();
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
  Event ev_[2];
  int k_ = 0;
  bool pend_ = false, issued_ = false;
  int64_t grows_ = 0, vgrows_ = 0;
};

}  // namespace wh_bind
