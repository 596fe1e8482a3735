// FM forward / backward and the single-shard native steps (module classes
// _hip.LinearStep and _hip.DifactoStep): one parameter-server shard trained
// in ONE native call per minibatch. The store is kv_store.h, the look-ahead
// localize the two steps share is localize_ahead.h, DifactoStep's guard is
// store_guard.h and LinearStep's own guard keeps its arithmetic in
// csrc/host/linear_guard_plan.h. The multi-shard step (psx_ops.cc) calls
// fm_forward, fm_backward and fm_grad_post here through ps_ops.h; everything
// else is local to this file. Host-only: validates tensors, sizes outputs
// and launches on the current PyTorch HIP stream.
#include "kv_store.h"
#include "localize_ahead.h"
#include "ps_ops.h"
#include "step_rt.h"
#include "store_guard.h"

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>

#include <cmath>
#include <cstring>
#include <memory>

#include "host/linear_guard_plan.h"

namespace wh_bind {
namespace {

// The row strides fm.hip has kernels for: 0 (linear) or 4 * 2^k <= 256 floats
// (a lane group of 1..64 lanes, a float4 each). Checked before anything
// else, so no tensor of a call with another stride is ever looked at.
void check_vstride(int64_t vstride) {
  TORCH_CHECK(vstride == 0 || (vstride >= 4 && vstride <= 256 && (vstride & (vstride - 1)) == 0),
              "vstride must be 0 or 4 * 2^k <= 256, got ", vstride);
}

// the forward's loss word: a 5th metric slot asks for the per-minibatch
// flipped accuracy (linear)
int loss_flags(int64_t loss, const Tensor& met) {
  return (int)loss | (met.numel() >= 5 ? 256 : 0);
}

}  // namespace

// --------------------------------------------------------------------- FM
// difacto: w_or_hdr = hdr [U,2], vc = [m, vstride]; linear: w_or_hdr = w [U]
std::vector<Tensor> fm_forward(const Tensor& offset, const Tensor& lid,
                               const c10::optional<Tensor>& val, const Tensor& w_or_hdr,
                               const c10::optional<Tensor>& vc, int64_t vstride,
                               const Tensor& label, int64_t loss, const Tensor& met) {
  check_vstride(vstride);
  CHECK_IN(offset, torch::kInt64);
  CHECK_IN(lid, torch::kInt32);
  CHECK_IN(w_or_hdr, torch::kFloat32);
  CHECK_IN(label, torch::kFloat32);
  CHECK_IN(met, torch::kFloat64);
  TORCH_CHECK(met.numel() >= 4, "met needs 4 doubles");
  const int64_t nrows = offset.numel() - 1;
  TORCH_CHECK(label.numel() == nrows, "label size mismatch");
  const float* vcp = nullptr;
  if (vstride > 0) {
    TORCH_CHECK(w_or_hdr.dim() == 2 && w_or_hdr.size(1) == 2, "hdr must be [U, 2]");
    TORCH_CHECK(vc.has_value() && vc->defined(), "vc required");
    CHECK_IN((*vc), torch::kFloat32);
    TORCH_CHECK(vc->numel() == 0 || (vc->dim() == 2 && vc->size(1) == vstride), "vc must be [m, vstride]");
    vcp = vc->numel() ? ptr<float>(*vc) : nullptr;
  }
  const float* vp = optptr<float>(val);
  c10::DeviceGuard g(offset.device());
  // py, dual, xv and the metric partials from ONE allocation (the views keep
  // it alive; four allocations were host time of the small-minibatch step)
  Carve c;
  const int64_t nxv = vstride > 0 ? nrows * vstride : 0;
  const int64_t o_py = c.add(nrows * 4), o_du = c.add(nrows * 4), o_xv = c.add(nxv * 4),
                o_pt = c.add(wh::fm_fwd_partials() * 8);
  c.alloc(offset.options());
  auto py = c.view(o_py, nrows, torch::kFloat32);
  auto dual = c.view(o_du, nrows, torch::kFloat32);
  auto xv = c.view(o_xv, nxv, torch::kFloat32);
  auto part = c.view(o_pt, wh::fm_fwd_partials(), torch::kFloat64);
  wh::fm_forward(nrows, ptr<int64_t>(offset), ptr<int32_t>(lid), vp, ptr<float>(w_or_hdr), vcp,
                 (int)vstride, ptr<float>(label), loss_flags(loss, met), ptr<float>(py),
                 ptr<float>(dual), vstride > 0 ? ptr<float>(xv) : nullptr, ptr<double>(met),
                 ptr<double>(part), ptr<unsigned int>(dev_ws(offset.device()).fwd_ticket),
                 cur_stream(offset));
  return {py, dual, xv};
}

namespace {

// The backward's outputs and scratch: {gw [U], gvc [vc_rows, vstride] (linear:
// empty), scratch [wh::fm_bwd_layout bytes]}. from_ws: the scratch is the
// current stream's grow-only workspace, good until the next backward on that
// stream; otherwise fresh memory (a plan outlives the call, and L-BFGS's
// spmv_t must not pin a data-set-sized buffer).
std::vector<Tensor> fm_bwd_alloc(const Tensor& csc_off, int64_t nnz, int64_t vc_rows,
                                 int64_t vstride, bool from_ws) {
  auto f32 = csc_off.options().dtype(torch::kFloat32);
  auto u8 = csc_off.options().dtype(torch::kUInt8);
  const int64_t U = csc_off.numel() - 1;
  const int64_t need = wh::fm_bwd_layout(U, nnz, (int)vstride, deterministic());
  Tensor fresh;
  Tensor& scratch = from_ws ? dev_ws(csc_off.device()).bwd_scratch[cur_stream(csc_off)] : fresh;
  if (!scratch.defined() || scratch.numel() < need)
    scratch = torch::empty({from_ws ? need + need / 4 : need}, u8);
  return {torch::empty({U}, f32),
          vstride > 0 ? torch::empty({vc_rows, vstride}, f32) : torch::empty({0}, f32), scratch};
}

// What the buffers `pl` (fm_bwd_alloc), the CSC's offsets and the sizes say
// of a backward; a launch adds the CSC's rows / values and the forward's
// inputs.
wh::FmBwdProblem fm_bwd_problem(const std::vector<Tensor>& pl, const Tensor& csc_off,
                                int64_t nnz, int64_t nrows, int64_t vstride) {
  wh::FmBwdProblem p = {};
  p.nuniq = csc_off.numel() - 1;
  p.nnz = nnz;
  p.nrows = nrows;
  p.csc_off = ptr<int64_t>(csc_off);
  p.vstride = (int)vstride;
  p.gw = ptr<float>(pl[0]);
  p.gvc = pl[1].numel() ? ptr<float>(pl[1]) : nullptr;
  p.deterministic = deterministic();
  return p;
}

// The fused update of a backward (wh::FmBwdProblem::fuse_v): the table's V
// and VG slabs and the store's hyper-parameters.
struct FmFuse {
  float *v, *vg;
  wh::DifactoHP hp;
};

// two_pass: plan without the look-back scan (count -> scan -> fill), the
// path of more keys than the scan has tiles
void fm_bwd_launch(const std::vector<Tensor>& pl, const Tensor& csc_off, const Tensor& csc_row,
                   const float* csc_val, const float* dual, const float* xv, const float* hdr,
                   const float* vc, int64_t vstride, int64_t nrows, wh::FmBwdPhase phase,
                   bool two_pass = false, const FmFuse* fuse = nullptr) {
  wh::FmBwdProblem p = fm_bwd_problem(pl, csc_off, csc_row.numel(), nrows, vstride);
  p.csc_row = ptr<int32_t>(csc_row);
  p.csc_val = csc_val;
  p.dual = dual;
  p.xv = xv;
  p.hdr = hdr;
  p.vc = vc;
  if (fuse) {
    p.fuse_v = fuse->v;
    p.fuse_vg = fuse->vg;
    p.fuse_hp = fuse->hp;
  }
  const wh::Lookback lb = lookback(csc_off.device());
  wh::fm_backward(p, pl[2].data_ptr(), two_pass ? nullptr : &lb, cur_stream(csc_off), phase);
}

void fm_bwd_check(const Tensor& csc_off, const Tensor& csc_row, const Tensor& w_or_hdr,
                  int64_t vstride) {
  check_vstride(vstride);
  CHECK_IN(csc_off, torch::kInt64);
  CHECK_IN(csc_row, torch::kInt32);
  CHECK_IN(w_or_hdr, torch::kFloat32);
  TORCH_CHECK(w_or_hdr.numel() == (csc_off.numel() - 1) * (vstride > 0 ? 2 : 1),
              "w/hdr must have U rows");
}

// the dual / xv dependent inputs of fm_backward and fm_backward_run; returns
// the rows of vc
int64_t fm_bwd_check_run(const Tensor& dual, const c10::optional<Tensor>& xv,
                         const c10::optional<Tensor>& vc, int64_t vstride) {
  CHECK_IN(dual, torch::kFloat32);
  if (vstride == 0) return 0;
  TORCH_CHECK(vc.has_value() && vc->defined() && xv.has_value() && xv->defined(), "vc/xv required");
  CHECK_IN((*vc), torch::kFloat32);
  CHECK_IN((*xv), torch::kFloat32);
  return vc->numel() ? vc->size(0) : 0;
}

// Where a kernel outside fm.hip (the single-shard open) writes the chunk plan
// of a backward whose buffers `pl` (fm_bwd_alloc) exist already.
wh::FmBwdPlanDst fm_bwd_plan_dst(const std::vector<Tensor>& pl, const Tensor& csc_off, int64_t nnz,
                                 int64_t nrows, int64_t vstride) {
  return wh::fm_bwd_plan_dst(fm_bwd_problem(pl, csc_off, nnz, nrows, vstride), pl[2].data_ptr());
}

// returns (gw [U], gvc [like vc]) (linear: gvc is empty); fuse (the native
// step only): single-chunk keys' gvc rows are not written, see FmBwdProblem;
// planned (the native step only): fm_bwd_alloc's buffers of this call, into
// which the open has written the chunk plan -- the backward then starts at
// the V-chunk bucketing instead of planning into buffers of its own
std::vector<Tensor> fm_backward_impl(const Tensor& csc_off, const Tensor& csc_row,
                                     const c10::optional<Tensor>& csc_val, const Tensor& dual,
                                     const c10::optional<Tensor>& xv, const Tensor& w_or_hdr,
                                     const c10::optional<Tensor>& vc, int64_t vstride,
                                     const FmFuse* fuse,
                                     const std::vector<Tensor>* planned = nullptr) {
  fm_bwd_check(csc_off, csc_row, w_or_hdr, vstride);
  const int64_t vrows = fm_bwd_check_run(dual, xv, vc, vstride);
  c10::DeviceGuard g(csc_off.device());
  TORCH_CHECK(!planned || (*planned)[1].numel() == vrows * vstride,
              "backward: gvc rows differ from vc's");
  std::vector<Tensor> own;
  if (!planned) own = fm_bwd_alloc(csc_off, csc_row.numel(), vrows, vstride, true);
  const std::vector<Tensor>& pl = planned ? *planned : own;
  fm_bwd_launch(pl, csc_off, csc_row, optptr<float>(csc_val), ptr<float>(dual),
                vstride > 0 ? optptr<float>(xv) : nullptr, ptr<float>(w_or_hdr),
                vstride > 0 ? optptr<float>(vc) : nullptr, vstride, dual.numel(),
                planned ? wh::FmBwdPhase::kBucketRun : wh::FmBwdPhase::kAll, false, fuse);
  return {pl[0], pl[1]};
}

}  // namespace

std::vector<Tensor> fm_backward(const Tensor& csc_off, const Tensor& csc_row,
                                const c10::optional<Tensor>& csc_val, const Tensor& dual,
                                const c10::optional<Tensor>& xv, const Tensor& w_or_hdr,
                                const c10::optional<Tensor>& vc, int64_t vstride) {
  return fm_backward_impl(csc_off, csc_row, csc_val, dual, xv, w_or_hdr, vc, vstride, nullptr);
}

// gvc [mcap, vstride]; m: device int64 tensor holding the live row count
void fm_grad_post(const Tensor& gvc, const Tensor& m, int64_t dim, double clip, double dropout,
                  int64_t seed, bool normalize) {
  CHECK_IN(gvc, torch::kFloat32);
  CHECK_IN(m, torch::kInt64);
  if (gvc.numel() == 0) return;
  TORCH_CHECK(gvc.dim() == 2, "gvc must be [m, vstride]");
  const int64_t vstride = gvc.size(1);
  c10::DeviceGuard g(gvc.device());
  auto s = cur_stream(gvc);
  Tensor sumsq;
  if (normalize) sumsq = torch::zeros({1}, gvc.options().dtype(torch::kFloat64));
  wh::fm_grad_post(ptr<int64_t>(m), gvc.size(0), ptr<float>(gvc), (int)vstride, (int)dim,
                   (float)clip, (float)dropout, (uint64_t)seed,
                   normalize ? ptr<double>(sumsq) : nullptr, s);
  if (normalize)
    wh::fm_grad_scale(ptr<int64_t>(m), gvc.size(0), ptr<float>(gvc), (int)vstride, (int)dim,
                      ptr<double>(sumsq), s);
}

namespace {

// Phase 1 of the backward on the CURRENT stream (the planning that needs no
// dual: chunk lists, zeroed multi-chunk gradients, V-chunk bucketing); the
// returned plan is finished by fm_backward_run (same CSC / header / vc).
// two_pass (tests): see fm_bwd_launch.
std::vector<Tensor> fm_backward_plan(const Tensor& csc_off, const Tensor& csc_row,
                                     const Tensor& w_or_hdr, int64_t vc_rows, int64_t nrows,
                                     int64_t vstride, bool two_pass) {
  fm_bwd_check(csc_off, csc_row, w_or_hdr, vstride);
  TORCH_CHECK(vc_rows >= 0 && nrows >= 0, "bad sizes");
  c10::DeviceGuard g(csc_off.device());
  auto pl = fm_bwd_alloc(csc_off, csc_row.numel(), vc_rows, vstride, false);
  fm_bwd_launch(pl, csc_off, csc_row, nullptr, nullptr, nullptr, ptr<float>(w_or_hdr), nullptr,
                vstride, nrows, wh::FmBwdPhase::kPlan, two_pass);
  return pl;
}

std::vector<Tensor> fm_backward_run(const std::vector<Tensor>& plan, const Tensor& csc_off,
                                    const Tensor& csc_row, const c10::optional<Tensor>& csc_val,
                                    const Tensor& dual, const c10::optional<Tensor>& xv,
                                    const Tensor& w_or_hdr, const c10::optional<Tensor>& vc,
                                    int64_t vstride) {
  fm_bwd_check(csc_off, csc_row, w_or_hdr, vstride);
  const int64_t vrows = fm_bwd_check_run(dual, xv, vc, vstride);
  // the plan is fm_bwd_alloc's fresh triple for this call's sizes. The
  // scratch must have exactly the layout's bytes: with U and vstride fixed
  // by gw / gvc, every region grows with nnz, so equal totals mean equal
  // region offsets, and the kernels find the lists where the plan wrote them
  TORCH_CHECK(plan.size() == 3, "fm_backward_run: not a backward plan");
  const Tensor &gw = plan[0], &gvc = plan[1], &scratch = plan[2];
  CHECK_IN(gw, torch::kFloat32);
  CHECK_IN(gvc, torch::kFloat32);
  CHECK_IN(scratch, torch::kUInt8);
  const int64_t U = csc_off.numel() - 1;
  TORCH_CHECK(gw.numel() == U, "fm_backward_run: U differs from the plan's");
  TORCH_CHECK(vstride > 0 ? gvc.dim() == 2 && gvc.size(0) == vrows && gvc.size(1) == vstride
                          : gvc.numel() == 0,
              "fm_backward_run: vc rows or vstride differ from the plan's");
  TORCH_CHECK(scratch.numel() == wh::fm_bwd_layout(U, csc_row.numel(), (int)vstride, deterministic()),
              "fm_backward_run: the plan was made for a CSC of another size");
  c10::DeviceGuard g(csc_off.device());
  // a plan allocated on a side stream is finished on this one, and the
  // caller may drop it as soon as the call returns
  for (const Tensor& t : plan)
    if (t.numel())
      c10::hip::HIPCachingAllocator::recordStream(
          t.storage().data_ptr(), c10::hip::getCurrentHIPStream(csc_off.device().index()));
  fm_bwd_launch(plan, csc_off, csc_row, optptr<float>(csc_val), ptr<float>(dual),
                vstride > 0 ? optptr<float>(xv) : nullptr, ptr<float>(w_or_hdr),
                vstride > 0 ? optptr<float>(vc) : nullptr, vstride, dual.numel(),
                wh::FmBwdPhase::kRun);
  return {gw, gvc};
}

// (tests) KVStore::difacto_open_pull with the backward's chunk plan emitted by
// the open, then the V-chunk bucketing: returns (slot, hdr, vc, vpos, plan),
// plan as fm_backward_plan returns it, for fm_backward_run. The plan is
// empty where the open fell back (DifactoStep then plans in the backward).
py::tuple difacto_open_pull_plan(KVStore& store, const Tensor& keys, bool insert,
                                 const c10::optional<Tensor>& cnt, const std::vector<double>& h,
                                 int64_t threshold, bool l1_shrk, int64_t seed, bool direct,
                                 const Tensor& csc_off, const Tensor& csc_row, int64_t nrows) {
  CHECK_IN(csc_off, torch::kInt64);
  CHECK_IN(csc_row, torch::kInt32);
  TORCH_CHECK(csc_off.numel() == keys.numel() + 1, "open_pull_plan: csc_off must have U + 1");
  c10::DeviceGuard g(keys.device());
  const int64_t vstride = store.vstride();
  check_vstride(vstride);
  TORCH_CHECK(vstride > 0, "open_pull_plan: an embedding store");
  const int64_t vrows = direct ? store.V_.size(0) : keys.numel();
  auto pl = fm_bwd_alloc(csc_off, csc_row.numel(), vrows, vstride, false);
  const wh::FmBwdPlanDst dst = fm_bwd_plan_dst(pl, csc_off, csc_row.numel(), nrows, vstride);
  bool planned = false;
  auto o = store.difacto_open_pull(keys, insert, cnt, h, threshold, l1_shrk, seed, direct, &dst,
                                   &planned);
  if (!planned) return py::make_tuple(o[0], o[1], o[2], o[3], std::vector<Tensor>());
  fm_bwd_launch(pl, csc_off, csc_row, nullptr, nullptr, nullptr, ptr<float>(o[1]), nullptr,
                vstride, nrows, wh::FmBwdPhase::kBucket);
  return py::make_tuple(o[0], o[1], o[2], o[3], pl);
}

// (tests) the chunk totals {scalar, V} of a backward plan, a device int64 [2]
Tensor fm_backward_plan_totals(const std::vector<Tensor>& plan, const Tensor& csc_off,
                               int64_t nnz, int64_t vstride) {
  TORCH_CHECK(plan.size() == 3, "not a backward plan");
  const wh::FmBwdPlanDst d = fm_bwd_plan_dst(plan, csc_off, nnz, 0, vstride);
  const int64_t base = reinterpret_cast<int64_t>(plan[2].data_ptr());
  const int64_t a = reinterpret_cast<int64_t>(d.tot_s) - base;
  const int64_t b = reinterpret_cast<int64_t>(d.tot_v) - base;
  auto i64 = plan[2].view(torch::kInt64);
  return torch::stack({i64[a / 8], i64[b / 8]});
}

int64_t vstride_for(int64_t dim) { return dim == 0 ? 0 : 4 * next_pow2((dim + 3) / 4); }

Tensor spmv_t(const Tensor& csc_off, const Tensor& csc_row, const c10::optional<Tensor>& csc_val,
              const Tensor& p) {
  CHECK_IN(csc_off, torch::kInt64);
  CHECK_IN(csc_row, torch::kInt32);
  CHECK_IN(p, torch::kFloat32);
  c10::DeviceGuard g(p.device());
  // the linear backward's chunked segmented sums (fm.hip k_chunk_plan /
  // k_bwd_scalar): a column is cut into chunks of at most a wave's width
  // and multi-chunk columns are summed across chunks, so a power-law head
  // (one Criteo value in a third of all rows) costs what its chunk count
  // costs -- one lane per column serialised such a column (298 ms per
  // L-BFGS gradient pass at 4M Criteo rows)
  auto pl = fm_bwd_alloc(csc_off, csc_row.numel(), 0, 0, false);
  fm_bwd_launch(pl, csc_off, csc_row, optptr<float>(csc_val), ptr<float>(p), nullptr, nullptr,
                nullptr, 0, p.numel(), wh::FmBwdPhase::kAll);
  return pl[0];
}

// frees coherent host memory that a kernel writes directly (hipHostMalloc)
struct HostFree {
  void operator()(void* p) const { (void)hipHostFree(p); }
};

// ------------------------------------------------------ native P=1 step
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
  // (the summaries' events and then the words they guard go with sum_, after
  // this body: no summary kernel is still to write freed memory)
  ~LinearStep() {
    ahead_.reset();
    for (Summ& m : sum_)
      if (m.ev) (void)hipEventSynchronize(m.ev);
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
    if (present(val)) {
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
    wh::lin_forward_strided(nrows, ptr<int64_t>(offset), lid, vp,
                            reinterpret_cast<const float*>(t.sl) + 2, 8, ptr<float>(label),
                            loss_flags(loss_, met), ptr<float>(fws), dual, ptr<double>(met),
                            ptr<double>(part), ptr<unsigned int>(dev_ws(keys.device()).fwd_ticket),
                            S);
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
      // (an empty csc_val, all ones, is no value array to the backward)
      auto bw = fm_backward(csc_off, csc_row, csc_val, fw[1], c10::nullopt, w, c10::nullopt, 0);
      ++pushes_;
      const double eta = (beta_ + std::sqrt((double)pushes_)) / alpha_;
      store_->linear_push(slot, bw[0], algo_, alpha_, beta_, l1_, l2_, eta);
    }
    return fw[0];
  }

  // drop a begun localize (end of a pass)
  void reset() { ahead_.reset(); }

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
  // ---- store guard without a per-step host wait: table summaries (keys,
  // failed inserts) are read when their event has completed (polled), the
  // key count in between is bounded by the inserts issued since; only a
  // table close to its load bound waits for the newest summary before
  // deciding to grow (nothing in flight references old slots: a grow is
  // stream-ordered before this step's inserts). The numbers -- the bound,
  // the grow target, when a summary is due, which summary counts -- are
  // wh::LinearGuardPlan's; here are the ring of summaries in flight and the
  // waits.
  struct Summ {
    // 4 words of coherent host memory the summary kernel writes directly (a
    // 32-byte hipMemcpyAsync to pinned memory cost ~40 us of host time);
    // declared before ev: freed after it
    std::unique_ptr<int64_t[], HostFree> h;
    Event ev;
    int64_t issued = 0;
    bool pending = false;
  };
  static constexpr int kSumm = 4;

  void guard_read(Summ& m) {
    const volatile int64_t* h = m.h.get();
    m.pending = false;
    TORCH_CHECK(h[1] == 0, "parameter store shard lost data: ", h[1], " failed inserts (table ",
                h[0], "/", store_->cap(), " keys)");
    plan_.summarised(h[0], m.issued);
  }
  void guard_poll(bool block) {
    for (Summ& m : sum_) {
      if (!m.pending) continue;
      if (block) WH_HIP_CHECK_HOST(hipEventSynchronize(m.ev));
      else if (hipEventQuery(m.ev) != hipSuccess) continue;
      guard_read(m);
    }
  }
  void guard_before(int64_t n_new) {
    guard_poll(false);
    if (plan_.grow_target(n_new, store_->cap(), max_load_) == store_->cap()) return;
    guard_poll(true);  // the exact count before growing
    const int64_t cap = plan_.grow_target(n_new, store_->cap(), max_load_);
    if (cap != store_->cap()) {
      store_->grow(cap);
      ++grows_;
    }
  }
  void guard_after(hipStream_t S, int64_t n_new, bool force = false) {
    if (!plan_.due(n_new, store_->cap(), max_load_, force)) return;
    Summ& m = sum_[sum_i_];
    sum_i_ = (sum_i_ + 1) % kSumm;
    if (m.pending) {  // (the GPU is kSumm steps behind: wait for the oldest)
      WH_HIP_CHECK_HOST(hipEventSynchronize(m.ev));
      guard_read(m);
    }
    if (!m.h) {
      void* p = nullptr;
      WH_HIP_CHECK_HOST(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(p, 0, 64);
      m.h.reset(static_cast<int64_t*>(p));
      m.ev.create();
    }
    wh::kv_summary(store_->table(), m.h.get(), S);
    WH_HIP_CHECK_HOST(hipEventRecord(m.ev, S));
    m.issued = plan_.issued;
    m.pending = true;
  }

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
  wh::LinearGuardPlan plan_;
  Summ sum_[kSumm];
  int sum_i_ = 0;
  int64_t grows_ = 0, pushes_ = 0;
};

// The single-shard DiFacto training / evaluation step in ONE native call
// (the Python twin, kept as the CPU path and the test oracle, is
// models/difacto.py DifactoLearner.process with WH_DIFACTO_NATIVE=0).
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
    // (val and csc_val may be empty, all ones: the kernels then get no value array)
    auto fw = fm_forward(offset, lid, val, hdr, vc, vs_, label, loss_, met);
    if (!train) auc_acc(fw[0], label, auc_sum);
    ht.mark(3);
    Tensor m = vpos.narrow(0, vpos.numel() - 1, 1);
    if (train && U > 0) {
      // (the slabs' addresses are this step's: the guard grows them before the open)
      const FmFuse fuse = {ptr<float>(store_->V_), ptr<float>(store_->VG_),
                           KVStore::dhp(hp_, threshold_, l1_shrk_, seed_)};
      // (the open's compact-pull fallback hands out a copy of the rows: unfused)
      const bool fuse_now = fused_v_ && vc.data_ptr() == store_->V_.data_ptr();
      auto bw = fm_backward_impl(csc_off, csc_row, csc_val, fw[1], fw[2], hdr, vc, vs_,
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

}  // namespace

void bind_fm(py::module_& m) {
  py::class_<LinearStep>(m, "LinearStep")
      .def(py::init<KVStore*, int64_t, double, double, double, double, int64_t, double, bool>(),
           py::arg("store"), py::arg("algo"), py::arg("alpha"), py::arg("beta"), py::arg("l1"),
           py::arg("l2"), py::arg("loss"), py::arg("max_load") = 0.7, py::arg("direct") = true,
           py::keep_alive<1, 2>())
      .def("step", &LinearStep::step, py::arg("keys"), py::arg("offset"), py::arg("val"),
           py::arg("label"), py::arg("train"), py::arg("met"), py::arg("auc_sum"),
           py::arg("next_keys") = py::none(), py::arg("next_offset") = py::none(),
           py::arg("next_val") = py::none(), py::arg("ready") = 0)
      .def("reset", &LinearStep::reset)
      .def("guard_sync", &LinearStep::guard_sync)
      .def_property_readonly("grows", &LinearStep::grows)
      .def_property_readonly("direct", [](const LinearStep& l) { return l.direct(); })
      .def_property("pushes", &LinearStep::pushes, &LinearStep::set_pushes);
  py::class_<DifactoStep>(m, "DifactoStep")
      .def(py::init<KVStore*, std::vector<double>, int64_t, bool, int64_t, int64_t,
                    std::vector<double>, double, bool, bool>(),
           py::arg("store"), py::arg("hp"), py::arg("threshold"), py::arg("l1_shrk"),
           py::arg("seed"), py::arg("loss"), py::arg("post"), py::arg("max_load"),
           py::arg("direct"), py::arg("fused_v") = true, py::keep_alive<1, 2>())
      .def("step", &DifactoStep::step, py::arg("keys"), py::arg("offset"), py::arg("val"),
           py::arg("label"), py::arg("train"), py::arg("data_pass"), py::arg("met"),
           py::arg("auc_sum"), py::arg("step"), py::arg("next_keys") = py::none(),
           py::arg("next_offset") = py::none(), py::arg("next_val") = py::none(),
           py::arg("ready") = 0)
      .def("reset", &DifactoStep::reset)
      .def("guard_sync", &DifactoStep::guard_sync)
      .def_property_readonly("direct", &DifactoStep::direct)
      .def_property_readonly("fused_v", &DifactoStep::fused_v)
      .def_property_readonly("grows", &DifactoStep::grows)
      .def_property_readonly("vgrows", &DifactoStep::vgrows);
  m.def("fm_forward", &fm_forward);
  m.def("set_cu_reserve", [](int64_t n) { wh::fm_set_cu_reserve((int)n); },
        "CUs the persistent FM kernels leave free for concurrent collectives");
  m.def("cu_reserve", []() { return (int64_t)wh::fm_cu_reserve(); });
  m.def("set_fm_bwd_pack", [](bool on) { wh::fm_set_bwd_pack(on); },
        "FM backward: pack small single-chunk keys, one lane group per key (default on)");
  m.def("fm_bwd_pack", []() { return wh::fm_bwd_pack(); });
  m.def("set_fm_fwd_depth", [](int64_t d) { wh::fm_set_fwd_depth((int)d); },
        "FM forward: 10 = a headline row's gathers in one batch; anything else = batches of 4 (default)");
  m.def("fm_fwd_depth", []() { return (int64_t)wh::fm_fwd_depth(); });
  m.def("fm_backward", &fm_backward);
  m.def("fm_backward_plan", &fm_backward_plan, py::arg("csc_off"), py::arg("csc_row"),
        py::arg("hdr"), py::arg("vc_rows"), py::arg("nrows"), py::arg("vstride"),
        py::arg("two_pass") = false);
  m.def("fm_backward_run", &fm_backward_run);
  m.def("difacto_open_pull_plan", &difacto_open_pull_plan, py::arg("store"), py::arg("keys"),
        py::arg("insert"), py::arg("cnt"), py::arg("h"), py::arg("threshold"),
        py::arg("l1_shrk"), py::arg("seed"), py::arg("direct"), py::arg("csc_off"),
        py::arg("csc_row"), py::arg("nrows"),
        "(tests) the open with the backward's chunk plan: (slot, hdr, vc, vpos, plan)");
  m.def("fm_backward_plan_totals", &fm_backward_plan_totals, py::arg("plan"),
        py::arg("csc_off"), py::arg("nnz"), py::arg("vstride"),
        "(tests) a backward plan's chunk totals {scalar, V}");
  m.def("fm_grad_post", &fm_grad_post);
  m.def("vstride_for", &vstride_for);
  m.def("spmv_t", &spmv_t, py::arg("csc_off"), py::arg("csc_row"), py::arg("csc_val"),
        py::arg("p"));
}

}  // namespace wh_bind
