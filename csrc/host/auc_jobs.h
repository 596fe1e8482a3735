// The job ledger of the host-thread AUC (csrc/bind/auc_ops.cc,
// WH_AUC_HOST_THREADS): which jobs are free, queued for a worker, or finished
// and waiting to be folded into their target's sum. Free of HIP and torch: the
// binding and the host self-test compile the same code. The binding owns what
// a job points to and does the copies and the waits: a submitter calls
// acquire, fills the job, submit, and later join; a worker take and finish.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <mutex>
#include <vector>

namespace wh {

struct AucJob {
  void* ev = nullptr;    // opaque here: the event after the job's copies
  float* buf = nullptr;  // opaque here: [cap] scores, then [cap] labels
  int64_t cap = 0, n = 0;
  const void* target = nullptr;  // the sum the result belongs to
  double result = 0;
  bool done = false;
};

class AucJobs {
 public:
  explicit AucJobs(int max_outstanding) : max_(max_outstanding) {}

  // A job for n examples: the first free one with cap >= n, else a fresh one
  // (cap == 0: the caller gives it a buffer). Smaller free jobs are left
  // alone, never regrown. Back-pressure: blocks while max_outstanding jobs are
  // acquired and not yet folded (the host falls this far behind only if its
  // threads are starved).
  AucJob* acquire(int64_t n) {
    std::unique_lock<std::mutex> lk(mu_);
    space_cv_.wait(lk, [&] { return outstanding_ < max_; });
    ++outstanding_;
    AucJob* j = nullptr;
    for (size_t k = 0; k < free_.size() && !j; ++k)
      if (free_[k]->cap >= n) {
        j = free_[k];
        free_.erase(free_.begin() + k);
      }
    if (!j) j = &all_.emplace_back();
    j->n = n;
    j->done = false;
    return j;
  }

  // after the job's copies and event are enqueued
  void submit(AucJob* j, const void* target) {
    std::lock_guard<std::mutex> lk(mu_);
    j->target = target;
    pending_.push_back(j);
    queue_.push_back(j);
    work_cv_.notify_one();
  }

  // a worker's next job, in submission order
  AucJob* take() {
    std::unique_lock<std::mutex> lk(mu_);
    work_cv_.wait(lk, [&] { return !queue_.empty(); });
    AucJob* j = queue_.front();
    queue_.pop_front();
    return j;
  }

  // Folds finished jobs into their target's sum in submission order (a
  // deterministic sum) and recycles them, so jobs never wait for a join. A
  // finished job behind an unfinished one stays pending and frees no space.
  void finish(AucJob* j, double result) {
    std::lock_guard<std::mutex> lk(mu_);
    j->result = result;
    j->done = true;
    while (!pending_.empty() && pending_.front()->done) {
      AucJob* f = pending_.front();
      pending_.pop_front();
      acc_[f->target] += f->result;
      free_.push_back(f);
      --outstanding_;
    }
    done_cv_.notify_all();
    space_cv_.notify_all();
  }

  // Waits until no unfolded job has this target; false when the target has no
  // sum (nothing was submitted for it since its last join), else its jobs'
  // results summed in submission order, and the sum is forgotten.
  bool join(const void* target, double* sum) {
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] {
      for (const AucJob* j : pending_)
        if (j->target == target) return false;
      return true;
    });
    auto it = acc_.find(target);
    if (it == acc_.end()) return false;
    *sum = it->second;
    acc_.erase(it);
    return true;
  }

 private:
  const int max_;
  std::mutex mu_;
  std::condition_variable work_cv_, done_cv_, space_cv_;
  std::deque<AucJob> all_;              // every job ever handed out (stable addresses)
  std::deque<AucJob*> queue_;           // submitted, not yet taken
  std::deque<AucJob*> pending_;         // submitted, not yet folded (submission order)
  std::map<const void*, double> acc_;   // folded sums per target
  std::vector<AucJob*> free_;
  int outstanding_ = 0;                 // acquired, not yet folded
};

}  // namespace wh
