// What one translation unit of the parameter-server family uses from another
// (hip_ops.cc, fm_ops.cc, psx_ops.cc, auc_ops.cc): declarations only, grouped
// by the unit that defines them. (The steps' streams and host timers are
// step_rt.h.)
#pragma once
#include "bind_common.h"

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

// ============================================================= auc_ops.cc
// auc_sum[0] += the minibatch's exact AUC: on the current stream, or (large
// minibatches) on the AUC side stream or host threads, joined by auc_join
void auc_acc(const Tensor& py, const Tensor& label, const Tensor& auc_sum);
void auc_acc_side(const Tensor& py, const Tensor& label, const Tensor& auc_sum);

}  // namespace wh_bind
