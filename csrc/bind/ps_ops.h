// What one translation unit of the parameter-server family uses from another
// (hip_ops.cc, fm_ops.cc, psx_ops.cc): declarations only, grouped by the unit
// that defines them.
#pragma once
#include "bind_common.h"

#include <array>
#include <map>

namespace wh_bind {

// ============================================================== fm_ops.cc
// FM forward / backward and the gradient post-processing, as the multi-shard
// step enqueues them (see the definitions)
std::vector<Tensor> fm_forward(const Tensor& offset, const Tensor& lid,
                               const c10::optional<Tensor>& val, const Tensor& w_or_hdr,
                               const c10::optional<Tensor>& vc, int64_t vstride,
                               const Tensor& label, int64_t loss, const Tensor& met);
std::vector<Tensor> fm_backward(const Tensor& csc_off, const Tensor& csc_row,
                                const c10::optional<Tensor>& csc_val, const Tensor& dual,
                                const c10::optional<Tensor>& xv, const Tensor& w_or_hdr,
                                const c10::optional<Tensor>& vc, int64_t vstride);
void fm_grad_post(const Tensor& gvc, const Tensor& m, int64_t dim, double clip, double dropout,
                  int64_t seed, bool normalize);

// ============================================================= hip_ops.cc
// Per-device persistent workspaces (allocated once, zero-initialised; the
// kernels that use them leave them in that state). Intentionally leaked: they
// must outlive every stream-ordered use and the process exit order. (Localize
// keeps a workspace of its own in localize_ops.cc.)
struct DevWs {
  Tensor lb;          // look-back scan granules + ticket (wh_lookback.h)
  Tensor auc;         // AUC bucket counters / min-max / area / ticket
  Tensor fwd_ticket;  // arrival counter of the forward's last-block reduction
  // the backward's scratch (wh::fm_bwd_layout bytes) per stream, grow-only:
  // reused in stream order by the next backward on the same stream (eight
  // allocations per call were ~20 us of host time, the bound of the
  // small-minibatch multi-shard step)
  std::map<hipStream_t, Tensor> bwd_scratch;
};
DevWs& dev_ws(const torch::Device& d);
// (its look-back scan, lookback(), is declared in kv_store.h, which uses it)

// ---- the worker / owner side of the multi-shard exchange
Tensor ps_records(const Tensor& uniq, const c10::optional<Tensor>& ucnt);
std::vector<Tensor> ps_c0(const Tensor& owner_cnt, const c10::optional<Tensor>& vcnt, int64_t P,
                          int64_t flag, bool loopback = false);
std::vector<Tensor> ps_unpack(const Tensor& rbuf, int64_t U, const Tensor& segS,
                              const Tensor& segHS, const Tensor& vrecv);
void ps_pack_gw(const Tensor& gw, const Tensor& gbuf, const Tensor& segS, const Tensor& segHS,
                const Tensor& vrecv);
Tensor ps_qpack(const Tensor& x, const Tensor& desc, int64_t rows, int64_t W, int64_t nb,
                int64_t seed);
void ps_qunpack(const Tensor& q, const Tensor& desc, int64_t W, int64_t nb, const Tensor& out);

// ---- the AUC chain
void auc_acc(const Tensor& py, const Tensor& label, const Tensor& auc_sum);
void auc_acc_side(const Tensor& py, const Tensor& label, const Tensor& auc_sum);

// ---- the native layer's own streams, one per device and role
enum OwnStream { kStreamLinearLs, kStreamPsxLs, kStreamPsxCs, kStreamPsxXs, kStreamAuc, kOwnStreams };
hipStream_t own_stream(int dev, int role);

// ---- WH_TIMING=step: host time per section of a native step
struct HostSplit {
  const char* name;
  double us[10] = {};
  int64_t calls = 0;
  bool abs = false;
  std::vector<std::array<int64_t, 11>> marks;
  explicit HostSplit(const char* n);
  ~HostSplit();
  HostSplit(const HostSplit&) = delete;
  HostSplit& operator=(const HostSplit&) = delete;
  void print() const;
};
class HostTimer {
 public:
  explicit HostTimer(HostSplit* h);
  void mark(int i);
  ~HostTimer();

 private:
  HostSplit* h_;
  std::chrono::steady_clock::time_point t_;
  bool rec_ = false;
  std::array<int64_t, 11> m_{};
};
// a split when WH_TIMING asks for one, else nullptr
HostSplit* host_split(const char* name);

}  // namespace wh_bind
